"""-m gpu: every loss kernel of csrc/loss.hip (and the warps it chains with) through the C ABI against fp64 autograd of the
oracle's functions, PER PIXEL, at the shapes where the kernels change path (tests/loss_parity.py: ragged tiles, the xcd_block()
remainder, one interior row, the 2x3 level, and BIG — past the 2048-block / 2048-tile caps, where every grid-stride loop and
chunked tile walk makes its second pass).

Tolerances: loss rel 1e-5; gradients max(2e-4, 2 x the fp32 torch-CPU oracle's own error on the same inputs) of the tensor's
max (the kernels use the ~1 ulp hardware rsq / rcp / exp / log forms); masks bit for bit.  No pixel is excused except the
photometric Charbonnier-kink pixels (|255 (im1 - im2w)| < 0.005 in fp64), whose share is capped at 5e-4.  Every test prints its
worst ratios (parity status)."""
import pytest
import torch

import loss_parity as P

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ERR_NULL, ERR_UNSUPPORTED = -1, -7


def _api():
    from unflow_amd import _lib
    return _lib.lib(), _lib


def _ok(status, where=""):
    from unflow_amd._lib import check
    check(status, where)


class _Dev:
    """Device copies of an input set and the buffers the kernels write: outputs start as NaN (a pixel a kernel skips stays NaN and
    fails every comparison), accumulators as zero."""

    def __init__(self, inp, dev):
        self.dev, self.inp = dev, inp
        self.N, self.B, self.H, self.W, self.fs = inp['N'], inp['B'], inp['H'], inp['W'], inp['fs']
        self.shape = (self.N, self.H, self.W)

    def t(self, key):
        return self.inp[key].to(self.dev).contiguous()

    def mask(self, n_mask, key='mask'):
        return self.inp[key + ('1' if n_mask == 1 else 'N')].to(self.dev).reshape(n_mask, self.H, self.W).contiguous()

    def im(self, ld):
        """[N,H,W,ld] image; the channels past 3 are NaN: a kernel that reads them poisons its result."""
        im = torch.full(self.shape + (ld,), float('nan'), device=self.dev)
        im[..., :3] = self.inp['im'].to(self.dev)
        return im

    def nan(self, *tail):
        return torch.full(self.shape + tail, float('nan'), device=self.dev)

    def acc(self):
        return torch.zeros(1, device=self.dev)


def _random_like(ref, dev, seed=99):
    """A buffer to accumulate into, of the gradient's own magnitude."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(ref.shape, generator=g) * ref.abs().max().item()).float().to(dev)


def _check_accumulated(got, buf, grad):
    """accumulate = 1: got = buf + grad.  The kernel may contract its last multiply with the add (one rounding instead of two):
    allow 2 ulp of the larger operand per element — a skipped or doubled pixel is off by |grad| itself."""
    tol = 2.0 ** -22 * (buf.abs() + grad.abs())
    bad = ((got - (buf + grad)).abs() > tol) | torch.isnan(got)
    assert not bool(bad.any()), ("accumulate", int(bad.sum()))


# ------------------------------------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("name,kind", P.SMOOTH_CASES)
@pytest.mark.parametrize("term", ['second_order', 'smooth_1st'])
def test_smoothness_kernels_per_pixel(term, name, kind, dev):
    lib, L = _api()
    d = _Dev(P.make_inputs(name, kind), dev)
    r64, r32 = P.ref_smooth(term, name, kind, F64), P.ref_smooth(term, name, kind, F32)
    bound, own = P.grad_bound(r32['d_flow'], r64['d_flow'])
    fn = lib.unflow_second_order_fwd_bwd if term == 'second_order' else lib.unflow_smooth_1st_fwd_bwd
    norm = d.B * d.H * d.W * (4 if term == 'second_order' else 2)
    flow, st = d.t('flow'), L.stream()

    def run(acc, gflow, accumulate):
        _ok(fn(L.ptr(flow), L.cf(d.fs), L.ptr(acc), L.ptr(gflow), accumulate, L.cf(3.0), L.cf(norm), d.N, d.H, d.W, st), term)

    acc, g0 = d.acc(), d.nan(2)
    run(acc, g0, 0)
    e_loss = P.check_loss(acc.item(), r64['loss'])
    e_grad = P.check_grad(g0, r64['d_flow'], bound)
    print("%s %s/%s: loss %.2e  d_flow %.2e (fp32 oracle %.2e, bound %.2e)" % (term, name, kind, e_loss, e_grad, own, bound))
    buf = _random_like(r64['d_flow'], dev)
    g1 = buf.clone()
    run(None, g1, 1)                                   # loss_acc = NULL
    _check_accumulated(g1, buf, g0)
    g2 = d.nan(2)
    run(None, g2, 0)
    assert torch.equal(g2, g0)                         # ... leaves the gradient bit-identical
    acc2 = d.acc()
    run(acc2, None, 0)                                 # d_flow = NULL leaves the loss
    P.check_loss(acc2.item(), r64['loss'])
    P.check_loss(acc2.item(), acc.item())


# ------------------------------------------------------------------------------------------------ photometric
@pytest.mark.parametrize("name,kind", P.WARP_CASES)
@pytest.mark.parametrize("n_mask", [1, 'N'])
def test_photometric_kernel_per_pixel(n_mask, name, kind, dev):
    lib, L = _api()
    n_mask = P.n_of(n_mask, name)
    d = _Dev(P.make_inputs(name, kind), dev)
    r64, r32 = P.ref_photometric(name, kind, n_mask, F64), P.ref_photometric(name, kind, n_mask, F32)
    kink = r64['kink']
    bound, own = P.grad_bound(r32['d_flow'], r64['d_flow'], kink)
    flow, mask, st = d.t('flow'), d.mask(n_mask), L.stream()
    norm = d.B * d.H * d.W * 3

    def run(im, ld, acc, gflow, accumulate):
        _ok(lib.unflow_photometric_fwd_bwd(L.ptr(im), ld, L.ptr(flow), L.cf(d.fs), L.ptr(mask), n_mask, L.ptr(acc), L.ptr(gflow),
                                           accumulate, L.cf(1.5), L.cf(norm), d.B, d.N, d.H, d.W, st), "photometric")

    grads = {}
    for ld in (3, 4):
        acc, g0 = d.acc(), d.nan(2)
        run(d.im(ld), ld, acc, g0, 0)
        e_loss = P.check_loss(acc.item(), r64['loss'])
        e_grad = P.check_grad(g0, r64['d_flow'], bound, kink)
        print("photometric %s/%s n_mask %d ld %d: loss %.2e  d_flow %.2e (fp32 oracle %.2e, bound %.2e, kink share %.1e)"
              % (name, kind, n_mask, ld, e_loss, e_grad, own, bound, kink.float().mean().item()))
        grads[ld] = g0
    assert torch.equal(grads[3], grads[4])             # the row pitch changes addresses only
    im = d.im(3)
    buf = _random_like(r64['d_flow'], dev)
    g1 = buf.clone()
    run(im, 3, None, g1, 1)
    _check_accumulated(g1, buf, grads[3])
    acc2 = d.acc()
    run(im, 3, acc2, None, 0)
    P.check_loss(acc2.item(), r64['loss'])


# ------------------------------------------------------------------------------------------------ Sobel gradient constancy
@pytest.mark.parametrize("name,kind", P.WARP_CASES)
@pytest.mark.parametrize("n_mask", [1, 'N'])
def test_gradient_loss_kernels_per_pixel(n_mask, name, kind, dev):
    lib, L = _api()
    n_mask = P.n_of(n_mask, name)
    d = _Dev(P.make_inputs(name, kind), dev)
    r64, r32 = P.ref_gradient(name, kind, n_mask, F64), P.ref_gradient(name, kind, n_mask, F32)
    bound, own = P.grad_bound(r32['d_im2w'], r64['d_im2w'])
    flow, mask, im2w, st = d.t('flow'), d.mask(n_mask), d.t('im2w'), L.stream()
    norm = d.B * d.H * d.W * 6

    def fwd_bwd(im, ld, warped):
        acc, gdiff, dimw = d.acc(), d.nan(6), d.nan(3)
        _ok(lib.unflow_gradient_loss_fwd(L.ptr(im), ld, L.ptr(warped), L.ptr(mask), n_mask, L.ptr(gdiff), L.ptr(acc), L.cf(2.0),
                                         L.cf(norm), d.N, d.H, d.W, st), "gradient_loss_fwd")
        _ok(lib.unflow_gradient_loss_bwd(L.ptr(gdiff), L.ptr(dimw), d.N, d.H, d.W, st), "gradient_loss_bwd")
        return acc, dimw

    outs = {}
    for ld in (3, 4):
        acc, dimw = fwd_bwd(d.im(ld), ld, im2w)
        e_loss = P.check_loss(acc.item(), r64['loss'])
        e_grad = P.check_grad(dimw, r64['d_im2w'], bound)
        print("gradient_loss %s/%s n_mask %d ld %d: loss %.2e  d_im2w %.2e (fp32 oracle %.2e, bound %.2e)"
              % (name, kind, n_mask, ld, e_loss, e_grad, own, bound))
        outs[ld] = dimw
    assert torch.equal(outs[3], outs[4])
    # ---- as the engine chains them: image_warp -> gradient loss -> image_warp backward, to the flow gradient
    c64, c32 = P.ref_gradient_chain(name, kind, n_mask, F64), P.ref_gradient_chain(name, kind, n_mask, F32)
    cbound, cown = P.grad_bound(c32['d_flow'], c64['d_flow'])
    im = d.im(3)
    warped = d.nan(3)
    _ok(lib.unflow_image_warp_fwd(L.ptr(im), 3, L.ptr(flow), L.cf(d.fs), L.ptr(warped), L.ptr(None), d.B, d.N, d.H, d.W, 3, st),
        "image_warp_fwd")
    acc, dimw = fwd_bwd(im, 3, warped)
    gflow = d.nan(2)
    _ok(lib.unflow_image_warp_bwd(L.ptr(dimw), L.ptr(im), 3, L.ptr(flow), L.cf(d.fs), L.ptr(None), L.ptr(gflow), 0, d.B, d.N, d.H,
                                  d.W, 3, st), "image_warp_bwd")
    e_loss = P.check_loss(acc.item(), c64['loss'])
    e_grad = P.check_grad(gflow, c64['d_flow'], cbound)
    print("gradient_loss chain %s/%s n_mask %d: loss %.2e  d_flow %.2e (fp32 oracle %.2e, bound %.2e)"
          % (name, kind, n_mask, e_loss, e_grad, cown, cbound))
    buf = _random_like(c64['d_flow'], dev)
    g1 = buf.clone()
    _ok(lib.unflow_image_warp_bwd(L.ptr(dimw), L.ptr(im), 3, L.ptr(flow), L.cf(d.fs), L.ptr(None), L.ptr(g1), 1, d.B, d.N, d.H,
                                  d.W, 3, st), "image_warp_bwd")
    _check_accumulated(g1, buf, gflow)


# ------------------------------------------------------------------------------------------------ masks + fb / occ / sym
@pytest.mark.parametrize("name,kind,mode,n_base", P.MASK_CASES)
def test_mask_terms_kernel_per_pixel(name, kind, mode, n_base, dev):
    lib, L = _api()
    n_base = P.n_of(n_base, name)
    d = _Dev(P.make_mask_inputs(name, kind), dev)
    flow, warped, fwarp, st = d.t('flow'), d.t('warped'), d.t('fwarp'), L.stream()
    base = d.mask(n_base, 'base') if n_base else None

    def run(w, mask_out, acc, gflow, gwarped, accumulate):
        _ok(lib.unflow_mask_terms(L.ptr(flow), L.ptr(warped), L.ptr(fwarp), L.ptr(base), n_base, L.cf(d.fs), mode, L.ptr(mask_out),
                                  L.ptr(acc), L.ptr(gflow), L.ptr(gwarped), accumulate, L.cf(w[0]), L.cf(w[1]), L.cf(w[2]), d.B,
                                  d.B, d.N, d.H, d.W, st), "mask_terms")

    for w in P.MASK_WEIGHTS:
        r64 = P.ref_mask_terms(name, kind, mode, n_base, w, F64)
        acc, mask_out = d.acc(), d.nan()
        if not w[0]:
            run(w, mask_out, acc, None, None, 0)
            P.check_mask(mask_out, r64['mask'])
            print("mask_terms %s/%s mode %d n_base %d w %s: loss %.2e" % (name, kind, mode, n_base, w, P.check_loss(acc.item(), r64['loss'])))
            continue
        r32 = P.ref_mask_terms(name, kind, mode, n_base, w, F32)
        gflow, gwarped = d.nan(2), d.nan(2)
        run(w, mask_out, acc, gflow, gwarped, 0)
        P.check_mask(mask_out, r64['mask'])
        e_loss = P.check_loss(acc.item(), r64['loss'])
        bf, of = P.grad_bound(r32['d_flow'], r64['d_flow'])
        bw, ow = P.grad_bound(r32['d_warped'], r64['d_warped'])
        e_f, e_w = P.check_grad(gflow, r64['d_flow'], bf), P.check_grad(gwarped, r64['d_warped'], bw)
        print("mask_terms %s/%s mode %d n_base %d w %s: loss %.2e  d_flow %.2e (fp32 oracle %.2e, bound %.2e)  d_warped %.2e "
              "(fp32 oracle %.2e, bound %.2e)" % (name, kind, mode, n_base, w, e_loss, e_f, of, bf, e_w, ow, bw))
        buf = _random_like(r64['d_flow'], dev)
        g1, gw1 = buf.clone(), d.nan(2)
        run(w, None, None, g1, gw1, 1)                 # mask_out = NULL, loss_acc = NULL
        _check_accumulated(g1, buf, gflow)
        assert torch.equal(gw1, gwarped)               # d_warped is overwritten either way


def test_mask_terms_null_argument_errors(dev):
    """The NULL-argument contract of unflow_mask_terms (include/unflow_hip.h): a term that needs an operand refuses to run without."""
    lib, L = _api()
    N, H, W = 2, 4, 5
    z = lambda *s: torch.zeros(*s, device=dev)
    flow, warped, fwarp, out, acc = z(N, H, W, 2), z(N, H, W, 2), z(N, H, W), z(N, H, W), z(1)
    st = L.stream()

    def call(flow=flow, warped=warped, fwarp=fwarp, mode=0, gflow=None, gwarped=None, w=(0.0, 1.0, 0.0)):
        return lib.unflow_mask_terms(L.ptr(flow), L.ptr(warped), L.ptr(fwarp), L.ptr(None), 1, L.cf(1.0), mode, L.ptr(out), L.ptr(acc),
                                     L.ptr(gflow), L.ptr(gwarped), 0, L.cf(w[0]), L.cf(w[1]), L.cf(w[2]), 1, 1, N, H, W, st)

    assert call() == 0
    assert call(flow=None) == ERR_NULL
    assert call(warped=None, w=(0.2, 0.0, 0.0)) == ERR_NULL          # fb needs warped_other
    assert call(warped=None, mode=1) == ERR_NULL                      # so does 'fb' occlusion masking
    assert call(fwarp=None, mode=2) == ERR_NULL                       # 'disocc' masking needs fwarp
    assert call(fwarp=None, w=(0.0, 0.0, 1.0)) == ERR_NULL            # and so does sym
    assert call(gflow=z(N, H, W, 2), w=(0.2, 0.0, 0.0)) == ERR_NULL   # a flow gradient of fb comes with d_warped
    assert call(warped=None, fwarp=None) == 0                         # occ alone on the outgoing mask needs neither
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ census
def _census_run(lib, L, d, g1, g2, mask, n_mask, D, weight=4.35):
    st = L.stream()
    acc, dist, dg = d.acc(), d.nan(), d.nan()
    norm = d.B * d.H * d.W
    _ok(lib.unflow_ternary_fwd(L.ptr(g1), L.ptr(g2), L.ptr(mask), n_mask, L.ptr(dist), L.ptr(acc), L.cf(weight), L.cf(norm), D, d.N,
                               d.H, d.W, st), "ternary_fwd")
    _ok(lib.unflow_ternary_bwd(L.ptr(g1), L.ptr(g2), L.ptr(mask), n_mask, L.ptr(dist), L.ptr(dg), L.cf(weight), L.cf(norm), D, d.N,
                               d.H, d.W, st), "ternary_bwd")
    return acc, dist, dg


@pytest.mark.parametrize("name,kind,D,n_mask", P.CENSUS_CASES)
def test_census_kernels_per_pixel(name, kind, D, n_mask, dev):
    lib, L = _api()
    n_mask = P.n_of(n_mask, name)
    d = _Dev(P.make_inputs(name, kind), dev)
    r64, r32 = P.ref_census(name, kind, D, n_mask, F64), P.ref_census(name, kind, D, n_mask, F32)
    g1, g2, mask, st = d.t('gray1'), d.t('gray2w'), d.mask(n_mask), L.stream()
    acc, dist, dg = _census_run(lib, L, d, g1, g2, mask, n_mask, D)
    e_loss = P.check_loss(acc.item(), r64['loss'])
    bd, od = P.grad_bound(r32['d_dist'], r64['d_dist'])
    bg, og = P.grad_bound(r32['d_gray2w'], r64['d_gray2w'])
    e_d, e_g = P.check_grad(dist, r64['d_dist'], bd), P.check_grad(dg, r64['d_gray2w'], bg)
    print("census %s/%s D %d n_mask %d: loss %.2e  dist_out %.2e (fp32 oracle %.2e, bound %.2e)  d_gray2w %.2e (fp32 oracle %.2e, "
          "bound %.2e)" % (name, kind, D, n_mask, e_loss, e_d, od, bd, e_g, og, bg))
    # the fused backward == ternary_bwd + warp_gray_bwd, bit for bit, accumulating and not
    im, flow = d.im(3), d.t('flow')
    for accumulate in (0, 1):
        buf = _random_like(r64['d_gray2w'].unsqueeze(-1).expand(*d.shape, 2), dev) if accumulate else d.nan(2)
        ga, gb = buf.clone(), buf.clone()
        _ok(lib.unflow_warp_gray_bwd(L.ptr(dg), L.ptr(im), 3, L.ptr(flow), L.cf(d.fs), L.ptr(ga), accumulate, d.B, d.N, d.H, d.W, st),
            "warp_gray_bwd")
        _ok(lib.unflow_ternary_warp_bwd(L.ptr(g1), L.ptr(g2), L.ptr(dist), L.ptr(im), 3, L.ptr(flow), L.cf(d.fs), L.ptr(gb),
                                        accumulate, d.B, D, d.N, d.H, d.W, st), "ternary_warp_bwd")
        assert not bool(torch.isnan(ga).any()) and torch.equal(ga, gb), accumulate


@pytest.mark.parametrize("N,H,W,D", [(2, 2, 37, 1), (2, 6, 40, 3), (2, 8, 37, 4), (2, 11, 8, 4)])
def test_census_without_interior_is_exactly_zero(N, H, W, D, dev):
    """H = 2D (or W = 2D): no pixel has its whole patch inside the image, so the term and its gradient are exactly 0."""
    lib, L = _api()
    g = torch.Generator().manual_seed(H * W)
    g1, g2 = (torch.rand(N, H, W, generator=g) * 255).to(dev), (torch.rand(N, H, W, generator=g) * 255).to(dev)
    mask = torch.ones(1, H, W, device=dev)
    d = _Dev(dict(N=N, B=N // 2, H=H, W=W, fs=1.0), dev)
    acc, dist, dg = _census_run(lib, L, d, g1, g2, mask, 1, D)
    assert acc.item() == 0.0
    assert torch.equal(dist, torch.zeros_like(dist)) and torch.equal(dg, torch.zeros_like(dg))


def test_census_max_distance_5_is_unsupported(dev):
    lib, L = _api()
    N, H, W = 2, 16, 40
    z = lambda *s: torch.zeros(*s, device=dev)
    g, m, o, acc, st = z(N, H, W), z(1, H, W), z(N, H, W), z(1), L.stream()
    im, flow, gflow = z(N, H, W, 3), z(N, H, W, 2), z(N, H, W, 2)
    assert lib.unflow_ternary_fwd(L.ptr(g), L.ptr(g), L.ptr(m), 1, L.ptr(o), L.ptr(acc), L.cf(1.0), L.cf(1.0), 5, N, H, W, st) == ERR_UNSUPPORTED
    assert lib.unflow_ternary_bwd(L.ptr(g), L.ptr(g), L.ptr(m), 1, L.ptr(o), L.ptr(o), L.cf(1.0), L.cf(1.0), 5, N, H, W, st) == ERR_UNSUPPORTED
    assert lib.unflow_ternary_warp_bwd(L.ptr(g), L.ptr(g), L.ptr(o), L.ptr(im), 3, L.ptr(flow), L.cf(1.0), L.ptr(gflow), 0, 1, 5, N, H,
                                       W, st) == ERR_UNSUPPORTED
    assert lib.unflow_ternary_fwd(L.ptr(g), L.ptr(g), L.ptr(m), 1, L.ptr(o), L.ptr(acc), L.cf(1.0), L.cf(1.0), 4, N, H, W, st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gray planes
@pytest.mark.parametrize("name,kind", P.GRAY_CASES)
def test_gray_kernels_per_pixel(name, kind, dev):
    """rgb_to_gray255, warp_gray_fwd and their fused form gray_pair against the oracle's gray of image_warp.  Bound: 1e-6 of the
    plane's max (the warps' forward tolerance) or twice the fp32 oracle's own error (flow * flow_scale rounds in fp32: at +-125 px
    that moves the sample point by 4e-6 px)."""
    lib, L = _api()
    d = _Dev(P.make_inputs(name, kind), dev)
    r64, r32 = P.ref_warp_gray(name, kind, F64), P.ref_warp_gray(name, kind, F32)
    flow, st = d.t('flow'), L.stream()
    outs = {}
    for ld in (3, 4):
        im = d.im(ld)
        g1, g2, p1, p2 = d.nan(), d.nan(), d.nan(), d.nan()
        _ok(lib.unflow_rgb_to_gray255(L.ptr(im), ld, L.ptr(g1), L.cl(d.N * d.H * d.W), st), "rgb_to_gray255")
        _ok(lib.unflow_warp_gray_fwd(L.ptr(im), ld, L.ptr(flow), L.cf(d.fs), L.ptr(g2), d.B, d.N, d.H, d.W, st), "warp_gray_fwd")
        _ok(lib.unflow_gray_pair(L.ptr(im), ld, L.ptr(flow), L.cf(d.fs), L.ptr(p1), L.ptr(p2), d.B, d.N, d.H, d.W, st), "gray_pair")
        for key, got in (('gray1', g1), ('gray2w', g2)):
            bound, own = P.grad_bound(r32[key], r64[key], floor=1e-6)
            e = P.check_grad(got, r64[key], bound)
            print("gray %s/%s ld %d %s: %.2e (fp32 oracle %.2e, bound %.2e)" % (name, kind, ld, key, e, own, bound))
        assert torch.equal(p1, g1) and torch.equal(p2, g2)          # the fused launch is the same arithmetic
        outs[ld] = (g1, g2)
    assert torch.equal(outs[3][0], outs[4][0]) and torch.equal(outs[3][1], outs[4][1])


# ------------------------------------------------------------------------------------------------ the default pyramid in four launches
def test_loss_pyramid_default_levels_past_the_caps(dev):
    """unflow_loss_pyramid_default over two levels: BIG, which fills every cap (2048 streaming blocks twice, 2048 census-forward
    blocks, 2100 census-backward tiles), so that the second level's blocks start at offsets 2048, 2048, 2048 and 2100, and a
    37x47 level after it.  Gradients bit-identical to the per-level entry points (themselves checked per pixel above), loss
    within rel 1e-5."""
    import ctypes
    lib, L = _api()
    big = P.make_inputs('BIG', 'm1.5')
    xcd = P.make_inputs('XCD', 'm4.0')
    N, B = big['N'], big['B']
    pick = [0, xcd['B']]                                  # one forward and one backward sample of XCD: a directed batch of 2
    st = L.stream()
    levels = []
    for inp, D, n_mask, sel in ((big, 1, 1, None), (xcd, 3, N, pick)):
        cut = (lambda t: t) if sel is None else (lambda t: t[sel])
        H, W = inp['H'], inp['W']
        mask = inp['mask1'] if n_mask == 1 else cut(inp['maskN'])
        lv = dict(H=H, W=W, D=D, n_mask=n_mask, fs=inp['fs'], im=cut(inp['im']).to(dev).contiguous(),
                  flow=cut(inp['flow']).to(dev).contiguous(), mask=mask.reshape(n_mask, H, W).to(dev).contiguous(),
                  tern=4.35 / (B * H * W), smooth=4.35 * 3.0 / (B * H * W * 4))
        levels.append(lv)

    def buffers(lv):
        f = lambda *tail: torch.full((N, lv['H'], lv['W']) + tail, float('nan'), device=dev)
        return dict(gray1=f(), gray2w=f(), dist=f(), gflow=f(2))

    # ---- per level
    acc_ref = torch.zeros(1, device=dev)
    ref = []
    for lv in levels:
        b = buffers(lv)
        H, W, D = lv['H'], lv['W'], lv['D']
        _ok(lib.unflow_second_order_fwd_bwd(L.ptr(lv['flow']), L.cf(lv['fs']), L.ptr(acc_ref), L.ptr(b['gflow']), 0, L.cf(lv['smooth']),
                                            L.cf(1.0), N, H, W, st), "second_order")
        _ok(lib.unflow_gray_pair(L.ptr(lv['im']), 3, L.ptr(lv['flow']), L.cf(lv['fs']), L.ptr(b['gray1']), L.ptr(b['gray2w']), B, N, H, W,
                                 st), "gray_pair")
        _ok(lib.unflow_ternary_fwd(L.ptr(b['gray1']), L.ptr(b['gray2w']), L.ptr(lv['mask']), lv['n_mask'], L.ptr(b['dist']),
                                   L.ptr(acc_ref), L.cf(lv['tern']), L.cf(1.0), D, N, H, W, st), "ternary_fwd")
        _ok(lib.unflow_ternary_warp_bwd(L.ptr(b['gray1']), L.ptr(b['gray2w']), L.ptr(b['dist']), L.ptr(lv['im']), 3, L.ptr(lv['flow']),
                                        L.cf(lv['fs']), L.ptr(b['gflow']), 1, B, D, N, H, W, st), "ternary_warp_bwd")
        ref.append(b)
    # ---- the four launches
    assert lib.unflow_sizeof_pyr_level() == ctypes.sizeof(L.PyrLevel)
    arr = (L.PyrLevel * len(levels))()
    got = []
    for k, lv in enumerate(levels):
        b = buffers(lv)
        got.append(b)
        arr[k] = L.PyrLevel(lv['im'].data_ptr(), lv['flow'].data_ptr(), b['gray1'].data_ptr(), b['gray2w'].data_ptr(),
                            lv['mask'].data_ptr(), b['dist'].data_ptr(), b['gflow'].data_ptr(), lv['H'], lv['W'], lv['n_mask'], lv['D'],
                            lv['fs'], lv['tern'], lv['smooth'])
    acc = torch.zeros(1, device=dev)
    _ok(lib.unflow_loss_pyramid_default(arr, len(levels), N, B, L.ptr(acc), 1, st), "loss_pyramid_default")
    torch.cuda.synchronize()
    for k in range(len(levels)):
        for key in ('gray1', 'gray2w', 'dist', 'gflow'):
            assert not bool(torch.isnan(got[k][key]).any()), (k, key)
            assert torch.equal(got[k][key], ref[k][key]), (k, key)
    print("loss pyramid: loss vs per-level %.2e" % P.check_loss(acc.item(), acc_ref.item()))
