"""The comparators and inputs of tests/test_frontend_kernels_gpu.py proven without a GPU (tests/frontend_parity.py): for every
case the fp32 torch-CPU evaluation of the oracle stands in for the kernel and passes every assertion the GPU tests make against
the fp64 reference; every share cap holds; every named mutant of the stand-ins fails on at least one small-shape case."""
import numpy as np
import pytest
import torch

import frontend_parity as Q

F32, F64 = torch.float32, torch.float64


def _fails(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ stn_affine
@pytest.mark.parametrize("case", Q.STN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_stn_fp32_oracle_passes(case):
    r32 = Q.ref_stn(case, F32)
    worst, own, bound, edge, outside = Q.check_stn(r32, case)
    assert worst == own and edge <= Q.STN_EDGE_SHARE_CAP and bound < 1e-3, (own, bound, edge)
    assert not bool(torch.isnan(Q.ref_stn(case, F64)).any())
    n_u, n_t, n_out = Q.stn_counts(case)
    Ho, Wo = Q.stn_out_size(case)
    assert tuple(r32.shape) == (n_out, Ho, Wo, case[1])
    if case[5] == 'far':
        # the two far samples: every pixel outside on both axes, floor(x) past the int range for scale 1e9
        _, theta = Q.make_stn_inputs(case)
        assert theta[2].abs().max() >= 1e9 and theta[2].abs().max() * Q.STN_SHAPES[case[0]][2] / 2 > 2.0 ** 31
        _, out = Q.stn_pixel_sets(case)
        assert bool(out[1].all()) and bool(out[2].all()) and not bool(out[0].all())
    print("stn %s: fp32 oracle %.1e  edge share %.1e  outside share %.2f" % (case, own, edge, outside))
    if case[0] != 'BIG':         # the transcription the mutants are applied to is the oracle, bit for bit
        U, theta = Q.make_stn_inputs(case)
        assert torch.equal(Q.standin_stn(U, theta, n_out, case[6]), r32)


def test_stn_cases_cover_the_forms():
    B, H, W = Q.STN_SHAPES['BIG']
    assert B * H * W > 2048 * 256 > (B - 1) * H * W
    C = Q.STN_CASES
    assert {(c[1], c[2], c[3]) for c in C} == set(Q.STN_LDS)
    assert {c[4] for c in C} == {'plain', 'mask', 'engine'} and {c[5] for c in C} == {'train', 'strong', 'far'}
    assert {c[6] for c in C if c[0] == 'RAGGED'} == {None, (11, 30), (40, 64)}
    assert {c[0] for c in C} == set(Q.STN_SHAPES) and sum(c[0] == 'BIG' for c in C) <= 4


@pytest.mark.parametrize("mutant", ['weights_first', 'step', 'nomod', 'halfpix', 'swap_bc'])
def test_stn_mutants_fail(mutant):
    hit = 0
    for case in Q.STN_CASES:
        if case[0] == 'BIG':
            continue
        U, theta = Q.make_stn_inputs(case)
        hit += _fails(Q.check_stn, Q.standin_stn(U, theta, Q.stn_counts(case)[2], case[6], mutant), case)
    assert hit >= 1, mutant
    print("stn mutant %s: rejected by %d small cases" % (mutant, hit))


def test_stn_nan_and_nonzero_outside_fail():
    case = ('RAGGED', 3, 3, 3, 'plain', 'far', None)
    r32 = Q.ref_stn(case, F32)
    bad = r32.clone()
    bad[1, 3, 4, 0] = 1e-30                # a far pixel: exactly 0 is required
    assert _fails(Q.check_stn, bad, case)
    bad = r32.clone()
    bad[0, 9, 20, 1] = float('nan')
    assert _fails(Q.check_stn, bad, case)


# ------------------------------------------------------------------------------------------------ photometric
@pytest.mark.parametrize("name", list(Q.PHOTO_SHAPES))
def test_photo_fp32_oracle_passes(name):
    for npar in ('B', 'N'):
        near0, lo, hi = Q.photo_pixel_sets(name, npar)
        assert lo >= 0.01 and hi >= 0.01, (lo, hi)                    # both clamps act
        for mean in (False, True):
            r32 = Q.ref_photo(name, npar, mean, F32)
            worst, own, bound, share = Q.check_photo(r32, name, npar, mean)
            assert worst == own and share <= Q.PHOTO_ZERO_SHARE_CAP and bound < 1e-5, (own, bound, share)
            if name != 'BIG':
                Q.check_photo(Q.standin_photo(name, npar, mean), name, npar, mean)
        print("photometric %s n_par %s: fp32 oracle %.1e  near-zero share %.1e  clamped low %.3f high %.3f" % (name, npar, own, share, lo, hi))
    im, _ = Q.make_photo_inputs(name)
    assert bool((im == 0).any()) and bool((im == 1).any())
    N, H, W = Q.PHOTO_SHAPES[name]
    assert N % 2 == 0 and (name != 'BIG' or N * H * W > 2048 * 256)


@pytest.mark.parametrize("mutant", ['gamma', 'clamp_after', 'colour_idx', 'noise_before', 'mean255', 'nomod'])
def test_photo_mutants_fail(mutant):
    hit = 0
    for name in ('RAGGED', 'ROW', 'TINY'):
        for npar in ('B', 'N'):
            for mean in (False, True):
                hit += _fails(Q.check_photo, Q.standin_photo(name, npar, mean, mutant), name, npar, mean)
    assert hit >= 1, mutant
    print("photometric mutant %s: rejected by %d of 12 small cases" % (mutant, hit))


# ------------------------------------------------------------------------------------------------ inference input
@pytest.mark.parametrize("u8", [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize("name", list(Q.INPUT_CASES))
def test_input_fp32_oracle_passes(name, u8):
    r32 = Q.ref_input(name, u8, F32)
    worst, own, bound = Q.check_input(r32, name, u8)
    assert worst == own and bound < 1e-4
    st, desc = Q.make_input_case(name, u8)
    frames, (H, W) = Q.INPUT_CASES[name]
    assert st.dtype == (np.uint8 if u8 else np.float32) and tuple(desc.shape) == (len(frames), 8) and desc.dtype == np.int32
    assert (desc[:, 5] == int(u8)).all() and (desc[:, 6:] == 0).all()
    if not u8:
        assert (st != np.floor(st)).mean() > 0.9                      # fractional parts
    if name == 'BIG':
        assert 2 * len(frames) * H * W > 2048 * 256
    else:
        assert torch.equal(Q.standin_input(name, u8), r32)            # the transcription the mutants are applied to
    print("inference_input %s %s: fp32 oracle %.1e" % (name, 'u8' if u8 else 'f32', own))


def test_input_frames_leave_the_buffer_on_every_side():
    Hm, Wm = Q.INPUT_STAGING
    F = Q.INPUT_FRAMES
    assert any(y0 < 0 for _, _, y0, _ in F) and any(x0 < 0 for _, _, _, x0 in F)
    assert any(y0 + h > Hm for h, _, y0, _ in F) and any(x0 + w > Wm for _, w, _, x0 in F)
    assert {(1, 1), (1, 40), (24, 1), (0, 0)} <= {(h, w) for h, w, _, _ in F}


@pytest.mark.parametrize("mutant", ['origin_sign', 'hi_max', 'edge_clamp', 'halfpix', 'align'])
def test_input_mutants_fail(mutant):
    hit = sum(_fails(Q.check_input, Q.standin_input(name, u8, mutant), name, u8) for name in ('N16x24', 'N32x64') for u8 in (False, True))
    assert hit >= 1, mutant


# ------------------------------------------------------------------------------------------------ inference output
@pytest.mark.parametrize("name", list(Q.OUT_CASES))
def test_output_fp32_oracle_passes(name):
    (Hm, Wm), _, frames, scale, metrics = Q.OUT_CASES[name]
    assert Q.out_blocks(Hm, Wm) == {'nb1': 1, 'nb4': 4, 'sat': 4, 'cap': 1024}[name[:3]]
    lo = hi = False
    outl = valid = 0
    for b, f in enumerate(frames):
        if f[0] == 0:
            continue
        got = Q.standin_output(name, b)
        res = Q.check_output_frame(got, name, b)
        assert res['worst'] == res['own'] and res['bound'] < 1e-4
        lo, hi = lo or bool((got['u16'][..., :2] == 0).any()), hi or bool((got['u16'][..., :2] == 65535).any())
        for o, v in zip(res['outliers'], res['valid']):
            outl, valid = outl + o, valid + v
            if v >= 200:
                assert 0.1 <= o / v <= 0.9, (name, b, o, v)
        print("inference_output %s frame %s: fp32 oracle %.1e  near-threshold share %.1e" % (name, f[:2], res['own'], res['near']))
    if name == 'saturate':
        assert lo and hi                                              # both saturations occur
    if metrics:
        assert 0.1 <= outl / valid <= 0.9
        assert {f[4] for f in frames if f[0]} == ({0, 1, 2} if len(frames) > 4 else {1, 2} if len(frames) > 1 else {2})
    if name == 'cap':
        assert Hm * Wm > 1024 * 1024 and (Hm * Wm + 1023) // 1024 > 1024


def test_output_frames():
    H, W = Q.OUT_NET
    assert any(h > H and w > W for h, w, *_ in Q.OUT_FRAMES_88)
    assert {(19, 45), (29, 37), (32, 64), (1, 1), (1, 45), (37, 83), (0, 0)} == {f[:2] for f in Q.OUT_FRAMES_88}
    for (Hm, Wm), frames in (((40, 88), Q.OUT_FRAMES_88), ((24, 40), Q.OUT_FRAMES_40)):
        assert all(h <= Hm and w <= Wm for h, w, *_ in frames)
        assert any(y0 < 0 or x0 < 0 or y0 + h > Hm or x0 + w > Wm for h, w, y0, x0, _ in frames)   # ground truth partly outside


@pytest.mark.parametrize("mutant", ['swap_r', 'one_stage', 'round', 'thr3', 'gt_origin'])
def test_output_mutants_fail(mutant):
    hit = 0
    for name in ('nb1_flow2', 'nb1_flow0', 'nb4_flow2', 'nb4_flow0', 'nb4_ragged'):
        for b, f in enumerate(Q.OUT_CASES[name][2]):
            if f[0]:
                hit += _fails(Q.check_output_frame, Q.standin_output(name, b, mutant), name, b)
    assert hit >= 1, mutant
    print("inference_output mutant %s: rejected by %d frames" % (mutant, hit))


# ------------------------------------------------------------------------------------------------ inference occlusion
@pytest.mark.parametrize("name", list(Q.OCC_CASES))
def test_occlusion_fp32_oracle_passes(name):
    (Hm, Wm), frames = Q.OCC_CASES[name]
    for b, f in enumerate(frames):
        if f[0] == 0:
            continue
        o_fw, o_bw = Q.standin_occlusion(name, b)
        counts = Q.occlusion_counts(o_fw.astype(bool), name, b)
        share, occ = Q.check_occlusion_frame(o_fw, o_bw, counts, name, b)
        if name == 'main':
            assert 0.1 <= occ <= 0.9, (f, occ)
            if f[0] * f[1] > 500:
                assert sum(counts) > 0 and min(counts) > 0
        else:
            assert occ == 0.0 and not o_fw.any() and not o_bw.any()    # the exact tie: visible
        print("inference_occlusion %s frame %s: near share %.1e  occluded %.2f" % (name, f[:2], share, occ))


def test_occlusion_tie_is_exact_in_both_precisions():
    c = Q.make_occlusion_case('tie')
    for dt in (F32, F64):
        fw, bw = c['fw'][:1, :5, :7].to(dt), c['bw'][:1, :5, :7].to(dt)
        mag = 0.01 * (Q.M.length_sq(fw) + Q.M.length_sq(bw)) + 0.5
        assert bool((mag == 2.0).all()) and bool((Q.M.length_sq(fw + Q.M.image_warp(bw, fw)) == 2.0).all())
        assert bool((Q.M.length_sq(bw + Q.M.image_warp(fw, bw)) == 2.0).all())
    assert float(np.float32(0.01) * np.float32(150.0) + np.float32(0.5)) == 2.0


@pytest.mark.parametrize("mutant", ['mag_warped', 'ge', 'clamp_max', 'same_field'])
def test_occlusion_mutants_fail(mutant):
    hit = 0
    for name in Q.OCC_CASES:
        for b, f in enumerate(Q.OCC_CASES[name][1]):
            if f[0]:
                o_fw, o_bw = Q.standin_occlusion(name, b, mutant)
                hit += _fails(Q.check_occlusion_frame, o_fw, o_bw, None, name, b)
    assert hit >= 1, mutant


def test_occlusion_counts_check_has_teeth():
    o_fw, o_bw = Q.standin_occlusion('main', 3)
    counts = Q.occlusion_counts(o_fw.astype(bool), 'main', 3)
    assert _fails(Q.check_occlusion_frame, o_fw, o_bw, [counts[0] + 1, counts[1], counts[2]], 'main', 3)
    # scored without the origin offset: other pixels, other counts
    h, w = Q.OCC_CASES['main'][1][3][:2]
    gt = Q.make_occlusion_case('main')['gt']
    ev = gt[0, 3, :h, :w].numpy() == 1
    gocc = ev & (gt[1, 3, :h, :w].numpy() == 0)
    assert [int((o_fw.astype(bool) & gocc).sum())] != counts[:1]
