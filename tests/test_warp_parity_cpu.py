"""The inputs, mirrors and comparators of tests/test_warp_kernels_gpu.py proven without a GPU (tests/warp_parity.py): the fp32
C oracle stands in for the kernels and must pass every assertion the GPU tests make against the fp64 mirrors; ranges and
indices are bit-equal; the constructed ten-wide footprints are what they claim to be; and every mutant of the mirrors — each
a way the kernels could be subtly wrong — is rejected by the same comparators at the same bounds."""
import numpy as np
import pytest
import torch

import warp_parity as P

F32, F64 = torch.float32, torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ forward_warp
@pytest.mark.parametrize("name,kind", P.FW_CASES)
def test_forward_warp_fp32_oracle_passes(name, kind):
    inp, r = P.fw_inputs(name, kind), P.fw_ref(name, kind)
    for key in ('out', 'd_flow'):
        bound, own = P.bound_of(r['o_' + key], r[key])
        assert bound < 1e-5, (key, bound)                 # fp32 noise, and the sensitivity the mutants below are judged at
        assert P.check(r['o_' + key], r[key], bound) == own
    P.check_ranges(r['o_ranges'], r['ranges'])
    P.check_rejected_zero(r['o_d_flow'], r['ok'])
    if kind != 'built':
        flat = inp['flow'].reshape(-1, 2)
        (z0, z1), (r0, r1) = P._blocks(flat.shape[0])
        assert (flat[z0:z1] == 0).all() and not r['ok'].reshape(-1)[r0:r1].any()
        assert r1 - r0 < 3 or (np.isinf(flat[r0:r1]).any() and np.isnan(flat[r0:r1]).any())
        assert r['ok'].mean() > 0.3


def test_case_shapes_reach_the_paths_they_claim():
    cdiv = lambda a, b: -(-a // b)
    tiles = lambda n, a, b: P.FW_SHAPES[n][0] * cdiv(P.FW_SHAPES[n][1], a) * cdiv(P.FW_SHAPES[n][2], b)
    assert tiles('RAGGED', 16, 64) == 6                    # per image one tile cut in x and one cut in x and y
    assert tiles('TILECAP', 16, 64) == 2050 > 2048
    assert tiles('BINCAP', 16, 64) == 2800 > 2048 and tiles('BINCAP', 32, 32) == 4900 > 4096 and cdiv(4900, 1024) == 5
    B, H, W = P.FW_SHAPES['WINDOW']
    assert H > 56 and W > 104 and H % 16 and W % 64 and H % 32 and W % 32
    B, H, W, C, s = P.DS_BIG
    assert B * (H // s) * (W // s) * C > 2048 * 256
    B, _, (oh, ow), C = P.RA_BIG
    assert B * oh * ow * C > 2048 * 256
    # NINE: a full 9 x 9 footprint exists, and only for sources that land on the centre
    for name in ('NINE', 'NINE2'):
        r = P.fw_ref(name, 'm1.5')['ranges']
        full = (r[..., 1] - r[..., 0] == 8) & (r[..., 3] - r[..., 2] == 8)
        assert full.any() == (name == 'NINE') and (~full & (r[..., 0] >= 0)).any()
    for name in ('TINY',):
        r = P.fw_ref(name, 'm1.5')
        whole = (r['ranges'][r['ok']] == [0, 2, 0, 1]).all(axis=1)  # clipped on all four sides: the whole image
        assert whole.any() and whole.mean() > 0.5


@pytest.mark.parametrize("name,kind", P.TORN_CASES)
def test_torn_fields_leave_the_window(name, kind):
    """Share of the accepted sources whose footprint leaves its source tile's window (the far path's load), counted from the
    mirror's footprints.  `More than half` cannot be had at these shapes: footprints are clipped to a 70 x 130 / 4 x 200 image
    that is hardly larger than the 56 x 104 window, which follows the tile's mean target.  Uniform +-60 px sends out 36 % on
    WINDOW and 14 % on BINCAP (u only); +-200 px sends out fewer on WINDOW (27 %: seven sources in eight are rejected) and
    47 % on BINCAP.  The sets stay at +-60 px; what is asserted is a tenth, against 0 - 5 % for the coherent fields."""
    share = P.fw_ref(name, kind)['far_share']
    assert share > 0.1, share
    assert P.fw_ref(name, 'm1.5' if name == 'BINCAP' else 'm4.0')['far_share'] < 0.05
    if name == 'BINCAP':      # 4 source tiles and 7 target tiles per image: the second pass of the fill (source tile 2048 on) and
        # of the gather (target tile 4096 on) has work where an image from 586 on has far sources
        assert P.fw_ref(name, kind)['far_tiles'][586:].sum() > 100


@pytest.mark.parametrize("name", ['TENTH', 'TENTHFAR'])
def test_tenth_sources_are_ten_wide(name):
    inp, r = P.fw_inputs(name, 'built'), P.fw_ref(name, 'built')
    fp = P.fw_footprints(inp['flow'])
    assert int(r['ok'].sum()) == len(P.TENTH_SOURCES[name])
    for (px, py), (tx, ty), rng in P.TENTH_SOURCES[name]:
        u, v = inp['flow'][0, py, px]
        assert np.float32(px) + u == np.float32(tx) and np.float32(py) + v == np.float32(ty)
        assert fp['tx'][0, py, px] == np.float32(tx) and fp['ty'][0, py, px] == np.float32(ty)
        assert r['ranges'][0, py, px].tolist() == list(rng)
        assert (rng[1] - rng[0] == 9) == (tx != 20.5) and (rng[3] - rng[2] == 9) == (ty != 8.5)
        assert r['o_ranges'][0, py, px].tolist() == list(rng)
    if name == 'TENTHFAR':
        assert r['far_share'] == 1.0                                    # both go through the binned gather
    else:
        assert r['far_share'] == 0.0                                    # all three stay in the window: the scatter's general path


def _fw_mutant_rejected(name, kind, keys=('out', 'd_flow'), **mut):
    inp, r = P.fw_inputs(name, kind), P.fw_ref(name, kind)
    out, d_flow, fp = P.fw_mirror(inp['flow'], inp['dout'], **mut)
    got = dict(out=_t(out).float(), d_flow=_t(d_flow).float())
    for key in keys:
        bound, _ = P.bound_of(r['o_' + key], r[key])
        with pytest.raises(AssertionError):
            P.check(got[key], r[key], bound)
    return fp, got


def test_mutant_nine_tap_cap_is_rejected_on_tenth():
    """The suspected kernel behaviour: at most nine taps per axis.  Rejected in the values and in d_flow; invisible where no
    footprint is ten wide (the mutant passes RAGGED: only a constructed input shows it)."""
    for name in ('TENTH', 'TENTHFAR'):
        _, got = _fw_mutant_rejected(name, 'built', cap=9)
        r = P.fw_ref(name, 'built')
        idx, g, m = P.worst_pixel(got['out'], r['out'])
        assert g == 0.0 and 1e-4 < m < 4e-4                 # the dropped tap: exp(-8) times its row weight
    inp, r = P.fw_inputs('RAGGED', 'm4.0'), P.fw_ref('RAGGED', 'm4.0')
    out, d_flow, _ = P.fw_mirror(inp['flow'], inp['dout'], cap=9)
    assert np.array_equal(out, r['out'].numpy()) and np.array_equal(d_flow, r['d_flow'].numpy())


def test_mutant_fp64_bounds_leave_no_tenth_column():
    fp, _ = _fw_mutant_rejected('TENTH', 'built', bounds64=True)
    with pytest.raises(AssertionError):
        P.check_ranges(P.fw_ranges(fp), P.fw_ref('TENTH', 'built')['ranges'])


@pytest.mark.parametrize("mut", [dict(strict_hi=True), dict(clip_w=True), dict(splat_rejected=True), dict(divisor=4.0),
                                 dict(seam=True)], ids=lambda m: next(iter(m)))
@pytest.mark.parametrize("name,kind", [('RAGGED', 'm1.5'), ('WINDOW', 'far')])
def test_mutants_of_the_splat_are_rejected(name, kind, mut):
    _fw_mutant_rejected(name, kind, **mut)


def test_mutant_gradient_without_dx_is_rejected():
    _fw_mutant_rejected('RAGGED', 'm1.5', keys=('d_flow',), grad_no_dx=True)


def test_forward_warp_comparators():
    r = P.fw_ref('RAGGED', 'm1.5')
    bound, _ = P.bound_of(r['o_out'], r['out'])
    P.check(r['out'].float(), r['out'], bound)
    bad = r['out'].float().clone()
    bad[2, 18, 44] += 1e-5 * r['out'].max().float()        # one corner pixel off by 1e-5 of the max
    with pytest.raises(AssertionError):
        P.check(bad, r['out'], bound)
    bad = r['out'].float().clone()
    bad[0, 0, 0] = float('nan')                             # a pixel the kernel never wrote
    with pytest.raises(AssertionError):
        P.check(bad, r['out'], bound)
    rng = r['ranges'].copy()
    rng[1, 3, 4, 1] += 1
    with pytest.raises(AssertionError):
        P.check_ranges(rng, r['ranges'])
    d = r['d_flow'].float().clone()
    P.check_rejected_zero(d, r['ok'])
    d[~torch.as_tensor(r['ok'])] = 1e-30
    with pytest.raises(AssertionError):
        P.check_rejected_zero(d, r['ok'])


def test_border_case_of_the_gradient():
    c = P.fw_border_case()
    bound, own = P.bound_of(c['o_d_flow'], c['d_flow'])
    assert bound < 1e-5 and bool(torch.isfinite(c['d_flow']).all())
    assert np.isnan(c['dout']).sum() == 3 * 20 * 2
    P.check_rejected_zero(c['o_d_flow'], c['ok'])


# ------------------------------------------------------------------------------------------------ backward_warp / image_warp
@pytest.mark.parametrize("shape,kind,C", P.BW_CASES)
def test_backward_warp_fp32_oracle_passes(shape, kind, C):
    inp, r = P.bw_inputs(shape, kind, C), P.bw_ref(shape, kind, C)
    P.check_ranges(r['o_xy0'], r['xy0'])
    bound, own = P.bound_of(r['o_out'], r['out'])
    assert bound < 1e-5
    P.check(r['o_out'], r['out'], bound)
    if kind != 'tiny':
        assert inp['exclude'].float().mean().item() <= P.EXCLUDE_CAP
        bound, own = P.bound_of(r['o_d_flow'], r['d_flow'], inp['exclude'])
        assert bound < 1e-5
        P.check(r['o_d_flow'], r['d_flow'], bound, inp['exclude'])
    if shape == 'COLUMN':
        assert inp['W'] == 1                                # x0 + 1 is never inside


def test_mutant_right_tap_at_the_last_column_is_rejected():
    inp, r = P.bw_inputs('RAGGED', 'm4.0', 2), P.bw_ref('RAGGED', 'm4.0', 2)
    assert (r['xy0'][..., 0] == inp['W'] - 1).any()
    out, d_flow, _ = P.bw_mirror(inp['im'], inp['flow'], inp['dout'], right_tap_at_edge=True)
    bound, _ = P.bound_of(r['o_out'], r['out'])
    with pytest.raises(AssertionError):
        P.check(_t(out).float(), r['out'], bound)
    bound, _ = P.bound_of(r['o_d_flow'], r['d_flow'], inp['exclude'])
    with pytest.raises(AssertionError):
        P.check(_t(d_flow).float(), r['d_flow'], bound, inp['exclude'])


@pytest.mark.parametrize("kind,C,shift", P.IW_CASES)
def test_image_warp_fp32_oracle_passes(kind, C, shift, oracle_lib):
    inp = P.iw_inputs(kind, C)
    r32, r64 = P.iw_ref(kind, C, shift, F32), P.iw_ref(kind, C, shift, F64)
    assert inp['exclude'].float().mean().item() <= P.EXCLUDE_CAP or kind == 'tiny'
    for key in ('out',) if kind == 'tiny' else ('out', 'd_im', 'd_flow'):
        ex = inp['exclude'] if key == 'd_flow' else None
        bound, own = P.bound_of(r32[key], r64[key], ex)
        assert bound < 1e-5, (key, bound)
        P.check(r32[key], r64[key], bound, ex)
    # the indices: the C oracle's (unshifted, flow already scaled) are the module's
    f = (inp['flow'] * np.float32(inp['fs'])).numpy()
    _, idx = oracle_lib.image_warp(inp['im'].numpy(), f, return_indices=True)
    if shift == 0:
        P.check_ranges(idx, P.iw_indices(kind, C, 0))
    else:
        B, H, W = inp['B'], inp['H'], inp['W']
        per = idx - (np.arange(B) * H * W).reshape(B, 1, 1, 1)
        exp = per + (((np.arange(B) + shift) % B) * H * W).reshape(B, 1, 1, 1)
        P.check_ranges(exp.astype(np.int32), P.iw_indices(kind, C, shift))


# ------------------------------------------------------------------------------------------------ downsample / resize_area
def test_area_weights_rows_sum_to_one_and_upsampling_splits_pixels():
    for n_in, n_out in [(5, 2), (7, 3), (3, 7), (37, 18), (53, 26), (1, 1), (310, 300), (420, 300)]:
        w = P.area_weights(n_in, n_out)
        assert torch.allclose(w.sum(1), torch.ones(n_out, dtype=F64), atol=1e-14) and bool((w >= 0).all())
    w = P.area_weights(3, 7)
    assert w[0].tolist() == [1.0, 0.0, 0.0]                                 # [0, 3/7): inside pixel 0
    assert abs(w[2, 0].item() - 1 / 3) < 1e-12 and abs(w[2, 1].item() - 2 / 3) < 1e-12     # [6/7, 9/7): a third / two thirds
    x = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]).view(1, 1, 5, 1)
    z = P.resize_area_ref(x, 1, 2).flatten()
    assert torch.allclose(z, torch.tensor([(1 + 2 + 1.5) / 2.5, (1.5 + 4 + 5) / 2.5], dtype=F64))


def test_downsample_oracle_is_the_box_mean(oracle_lib):
    for C, s in P.DS_GENERIC_CASES:
        im = P.ds_image(2, 3 * s, 5 * s, C)
        ref = oracle_lib.downsample(im, s)
        m = im.astype(np.float64).reshape(2, 3, s, 5, s, C).mean(axis=(2, 4))
        assert ref.shape == (2, 3, 5, C) and np.abs(ref - m).max() < 1e-6
        assert not (C == 3 and s in (2, 4))                 # none of them is taken by the three-channel kernel
