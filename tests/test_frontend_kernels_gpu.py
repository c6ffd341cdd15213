"""-m gpu: the kernels at the two ends of the pipeline through the C ABI, per element, against fp64 evaluations of the oracle's own
expressions (tests/frontend_parity.py holds the shapes, inputs, references, comparators and exclusions;
tests/test_frontend_parity_cpu.py proves them without a GPU):

* unflow_stn_affine_fwd: both specialised templates and the generic one (ld_u > C, ld_out > C, NaN in the unread channels, the
  output padding checked untouched), n_u = 1 / n_theta = B, the engine's n_u = 2B / n_theta = B, out_size below and above
  (H, W), training, strong and far-out thetas (exactly 0 where both coordinates are outside), BIG past the 2048-block cap.
* unflow_photometric_augment: N = 2B with n_par = B and N, ld_in / ld_out 3 and 4, with and without the mean, draws at which
  both clamps act, exact 0 and 1 in the image.
* unflow_inference_input / _input_frames: hand-written desc rows whose frames leave the staging row on every side, frames of
  height / width 1, an empty slot, uint8 and fp32, the operand planes for 3 and 1 planes, BIG past the cap.
* unflow_inference_output: one block, four blocks and the 1024-block cap; flow2, flow0 and a non-dyadic flow; a frame larger
  than the network; the 16-bit encoding with both saturations; error sums, mask sums and outlier counts for 0, 1 and 2 maps.
* unflow_inference_occlusion: frames of height / width 1, the whole row, far flows whose taps clamp at the frame, an exact tie
  of the inequality, TP / FP / FN.

Outputs start as NaN or a sentinel.  Every test prints its worst ratios (parity status)."""
import numpy as np
import pytest
import torch

import frontend_parity as Q

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float('nan')


def _api():
    from unflow_amd import _lib
    return _lib.lib(), _lib


def _ok(status, where=""):
    from unflow_amd._lib import check
    check(status, where)


def _padded(t, ld, dev, pad_value):
    """t [.., C] as a [.., ld] device tensor with pad_value in the columns past C."""
    out = torch.full(tuple(t.shape[:-1]) + (ld,), pad_value, device=dev)
    out[..., :t.shape[-1]] = t.to(dev)
    return out.contiguous()


# ------------------------------------------------------------------------------------------------ stn_affine
@pytest.mark.parametrize("case", Q.STN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_stn_affine_per_element(case, dev):
    lib, L = _api()
    name, C, ld_u, ld_out, _, _, _ = case
    _, H, W = Q.STN_SHAPES[name]
    n_u, n_t, n_out = Q.stn_counts(case)
    Ho, Wo = Q.stn_out_size(case)
    U, theta = Q.make_stn_inputs(case)
    Ud, th = _padded(U, ld_u, dev, NAN), theta.to(dev).contiguous()
    out = torch.full((n_out, Ho, Wo, ld_out), NAN, device=dev)         # a pixel the kernel skips stays NaN
    out[..., C:] = Q.SENTINEL
    _ok(lib.unflow_stn_affine_fwd(L.ptr(Ud), n_u, ld_u, L.ptr(th), n_t, L.ptr(out), ld_out, n_out, H, W, C, Ho, Wo, L.stream()),
        "stn_affine")
    torch.cuda.synchronize()
    assert bool((out[..., C:] == Q.SENTINEL).all()), "padding written"
    worst, own, bound, edge, outside = Q.check_stn(out[..., :C], case)
    assert edge <= Q.STN_EDGE_SHARE_CAP
    print("stn_affine %s: %.2e (fp32 oracle %.2e, bound %.2e)  excluded share %.1e  exactly-0 share %.2f"
          % ("-".join(str(v) for v in case), worst, own, bound, edge, outside))


# ------------------------------------------------------------------------------------------------ photometric
@pytest.mark.parametrize("name", list(Q.PHOTO_SHAPES))
def test_photometric_augment_per_element(name, dev):
    lib, L = _api()
    N, H, W = Q.PHOTO_SHAPES[name]
    im, draws = Q.make_photo_inputs(name)
    mean3 = (L.ctypes.c_float * 3)(*Q.CHANNEL_MEAN)
    worst_all = own_all = 0.0
    for npar, ld_in, ld_out, with_mean in (Q.PHOTO_BIG_FORMS if name == 'BIG' else Q.PHOTO_FORMS):
        n_par = Q.photo_npar(name, npar)
        d = {k: v[:n_par].to(dev).contiguous() for k, v in draws.items()}
        imd = _padded(im, ld_in, dev, NAN)
        out = torch.full((N, H, W, ld_out), NAN, device=dev)
        _ok(lib.unflow_photometric_augment(L.ptr(imd), ld_in, L.ptr(out), ld_out, L.ptr(d['contrast']), L.ptr(d['brightness']),
                                           L.ptr(d['colour']), L.ptr(d['gamma']), L.ptr(d['noise']), n_par,
                                           mean3 if with_mean else None, N, H, W, L.stream()), "photometric")
        torch.cuda.synchronize()
        if ld_out > 3:
            assert bool((out[..., 3:] == 0).all()), "the fourth channel is exactly 0"
        worst, own, bound, share = Q.check_photo(out[..., :3], name, npar, with_mean)
        assert share <= Q.PHOTO_ZERO_SHARE_CAP
        worst_all, own_all = max(worst_all, worst), max(own_all, own)
    print("photometric %s %dx%dx%d: abs %.2e (fp32 oracle %.2e, bound max(2e-6, 2 x oracle))" % (name, N, H, W, worst_all, own_all))


# ------------------------------------------------------------------------------------------------ inference input
@pytest.mark.parametrize("u8", [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize("name", list(Q.INPUT_CASES))
def test_inference_input_per_element(name, u8, dev):
    from unflow_amd.core import layers as Lay
    lib, L = _api()
    frames, (H, W) = Q.INPUT_CASES[name]
    B = len(frames)
    Hm, Wm = Q.INPUT_STAGING
    staged, desc = Q.make_input_case(name, u8)
    st, dd = torch.from_numpy(staged).to(dev), torch.from_numpy(desc).to(dev)
    mean3 = (L.ctypes.c_float * 3)(*Q.CHANNEL_MEAN)
    first = None
    for n_planes in (3, 1):
        x0 = torch.full((2 * B, H, W, 4), NAN, device=dev)
        pl = torch.full((n_planes, 2 * B, H, W, 4), 0x1234, dtype=torch.int16, device=dev)
        _ok(lib.unflow_inference_input(L.ptr(st), L.ptr(dd), B, Hm, Wm, H, W, L.ptr(x0), mean3, L.planes_of(pl), L.stream()),
            "inference_input")
        torch.cuda.synchronize()
        assert bool((x0[..., 3] == 0).all()), "the fourth channel is exactly 0"
        want = torch.zeros_like(pl)
        Lay.planes_from_f32(x0, want, C=4)
        torch.cuda.synchronize()
        assert torch.equal(pl, want), ("operand planes", n_planes)
        if first is None:
            first, first_pl = x0, pl
            worst, own, bound = Q.check_input(x0[..., :3], name, u8)
        else:
            assert torch.equal(x0, first)
    # the sequence entry: the same frames, one per row, bit-identical to the pair kernel's rows
    for k in range(2):
        rows = torch.full((B + 2, H, W, 4), Q.SENTINEL, device=dev)
        pl = torch.full((3, B + 2, H, W, 4), 0x1234, dtype=torch.int16, device=dev)
        _ok(lib.unflow_inference_input_frames(L.ptr(st[k]), L.ptr(dd), B, Hm, Wm, H, W, L.ptr(rows[1:]), mean3,
                                              L.planes_of(pl[:, 1:]), L.stream()), "inference_input_frames")
        torch.cuda.synchronize()
        assert torch.equal(rows[1:B + 1], first[k * B:(k + 1) * B]) and torch.equal(pl[:, 1:B + 1], first_pl[:, k * B:(k + 1) * B])
        for r in (0, B + 1):
            assert bool((rows[r] == Q.SENTINEL).all()) and bool((pl[:, r] == 0x1234).all())
    print("inference_input %s %s -> %dx%d: %.2e (fp32 oracle %.2e, bound %.2e)" % (name, 'u8' if u8 else 'f32', H, W, worst, own, bound))


# ------------------------------------------------------------------------------------------------ inference output
def _launch_output(name, dev):
    lib, L = _api()
    (Hm, Wm), (fh, fw), frames, scale, metrics = Q.OUT_CASES[name]
    H, W = Q.OUT_NET
    B = len(frames)
    c = Q.make_output_case(name)
    flow, desc = c['flow'].to(dev).contiguous(), torch.from_numpy(c['desc']).to(dev)
    gt = c['gt'].to(dev).contiguous() if metrics else None
    mask = c['mask'].to(dev).contiguous() if metrics else None
    nb = lib.unflow_inference_output_blocks(Hm, Wm)
    assert nb == Q.out_blocks(Hm, Wm)
    out = torch.full((B, Hm, Wm, 2), Q.SENTINEL, device=dev)
    u16 = torch.full((B, Hm, Wm, 3), Q.OUT_U16_SENTINEL, dtype=torch.int16, device=dev)
    partial = torch.zeros(B * nb * 6, dtype=F64, device=dev)
    ticket = torch.zeros(B, dtype=torch.int32, device=dev)
    sums = torch.zeros(B, 2, 2, dtype=F64, device=dev)
    counts = torch.zeros(B, 2, dtype=torch.int32, device=dev)
    _ok(lib.unflow_inference_output(L.ptr(flow), fh, fw, L.cf(scale), H, W, L.ptr(desc), B, Hm, Wm, L.ptr(out), L.ptr(u16),
                                    L.ptr(gt), L.ptr(mask), L.ptr(partial), L.ptr(ticket), L.ptr(sums), L.ptr(counts), L.stream()),
        "inference_output")
    torch.cuda.synchronize()
    assert bool((ticket == 0).all()), "ticket back at 0"
    return out.cpu(), u16.cpu(), sums.cpu(), counts.cpu()


@pytest.mark.parametrize("name", list(Q.OUT_CASES))
def test_inference_output_per_element(name, dev):
    (Hm, Wm), _, frames, scale, metrics = Q.OUT_CASES[name]
    out, u16, sums, counts = _launch_output(name, dev)
    again = _launch_output(name, dev)
    assert all(torch.equal(a, b) for a, b in zip((out, u16, sums, counts), again)), "two launches are bit-identical"
    u16n = u16.numpy().view(np.uint16)
    lo = hi = False
    for b, (h, w, _, _, nmaps) in enumerate(frames):
        # nothing outside (h, w) is written; an empty slot and the maps a sample does not have leave their sums alone
        assert bool((out[b, h:] == Q.SENTINEL).all()) and bool((out[b, :h, w:] == Q.SENTINEL).all())
        assert (u16n[b, h:] == Q.OUT_U16_SENTINEL).all() and (u16n[b, :h, w:] == Q.OUT_U16_SENTINEL).all()
        k0 = nmaps if (metrics and h) else 0
        assert bool((sums[b, k0:] == 0).all()) and bool((counts[b, k0:] == 0).all())
        if h == 0:
            continue
        got = dict(flow=out[b, :h, :w], u16=u16n[b, :h, :w],
                   maps=[(sums[b, k, 0].item(), sums[b, k, 1].item(), int(counts[b, k])) for k in range(k0)])
        res = Q.check_output_frame(got, name, b)
        lo, hi = lo or bool((got['u16'][..., :2] == 0).any()), hi or bool((got['u16'][..., :2] == 65535).any())
        print("inference_output %s frame %dx%d: %.2e (fp32 oracle %.2e, bound %.2e)  near-threshold share %.1e"
              % (name, h, w, res['worst'], res['own'], res['bound'], res['near']))
    if name == 'saturate':
        assert lo and hi, "both saturations occur"


# ------------------------------------------------------------------------------------------------ inference occlusion
def _launch_occlusion(name, dev, with_gt=True):
    lib, L = _api()
    (Hm, Wm), frames = Q.OCC_CASES[name]
    B = len(frames)
    c = Q.make_occlusion_case(name)
    fw, bw = c['fw'].to(dev).contiguous(), c['bw'].to(dev).contiguous()
    desc = torch.from_numpy(c['desc']).to(dev)
    gt = c['gt'].to(dev).contiguous() if with_gt else None
    occ = torch.full((2, B, Hm, Wm), Q.OCC_SENTINEL, dtype=torch.uint8, device=dev)
    counts = torch.full((B, 3), 99, dtype=torch.int32, device=dev)
    _ok(lib.unflow_inference_occlusion(L.ptr(fw), L.ptr(bw), L.ptr(desc), B, Hm, Wm, L.ptr(gt), L.ptr(occ[0]), L.ptr(occ[1]),
                                       L.ptr(counts), L.stream()), "inference_occlusion")
    torch.cuda.synchronize()
    return occ.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("name", list(Q.OCC_CASES))
def test_inference_occlusion_per_pixel(name, dev):
    (Hm, Wm), frames = Q.OCC_CASES[name]
    occ, counts = _launch_occlusion(name, dev)
    occ2, counts2 = _launch_occlusion(name, dev)
    assert np.array_equal(occ, occ2) and np.array_equal(counts, counts2)
    occ_n, counts_n = _launch_occlusion(name, dev, with_gt=False)      # not scored: the same masks, counts zero
    assert np.array_equal(occ, occ_n) and (counts_n == 0).all()
    for b, (h, w, _, _, nmaps) in enumerate(frames):
        assert (occ[:, b, h:] == Q.OCC_SENTINEL).all() and (occ[:, b, :h, w:] == Q.OCC_SENTINEL).all()   # nothing outside the frame
        if h == 0 or nmaps < 2:
            assert (counts[b] == 0).all()
        if h == 0:
            continue
        share, frac = Q.check_occlusion_frame(occ[0, b, :h, :w], occ[1, b, :h, :w], counts[b] if nmaps >= 2 else None, name, b)
        print("inference_occlusion %s frame %dx%d: masks equal outside a near-threshold share of %.1e; occluded %.2f; TP FP FN %s"
              % (name, h, w, share, frac, [int(v) for v in counts[b]]))
