"""Input builders, fp64 references and comparators of the per-pixel loss / warp parity tests (tests/test_loss_kernels_gpu.py,
proven without a GPU by tests/test_loss_parity_cpu.py).  Not a test file.

References are autograd over the oracle's own functions (oracle/model_ref.py) — evaluated in fp64 as THE reference and in
fp32 as the yardstick of what fp32 arithmetic can deliver on the same inputs.  Every input is an fp32 tensor; the oracle gets
its .double(), so both sides see exactly the same numbers.

Directed batch: N = 2B samples, sample n's second image / partner is sample (n + B) % N (pair_shift = B)."""
import contextlib
import functools

import torch

from oracle import model_ref as M

# name -> (N, H, W); what each one is for: see DESIGN.md (parity status)
SHAPES = {
    'RAGGED': (4, 19, 45),      # ragged against the 8x32 census tiles and the 64x4 warp tiles; < 16 blocks
    'XCD': (6, 37, 47),         # 10,434 px: 41 streaming blocks (41 % 8 = 1), 60 census tiles (60 % 8 = 4): xcd_block() remainder
    'ROW': (2, 7, 70),          # with D = 3: exactly one interior row
    'TINY': (2, 2, 3),          # the deepest engine level (census at D = 0 only: the oracle needs H, W > 2D)
    'BIG': (2, 333, 795),       # 529,470 px > 2048 * 256; 2100 census tiles and 2184 warp tiles > 2048: every second pass
}
# input sets: seed, flow magnitude (flow = randn * mag), a fifth of the flows at +-50 px (the clamped taps of the warps)
SETS = {
    'm1.5': dict(seed=5, mag=1.5, far=False),
    'm4.0': dict(seed=6, mag=4.0, far=False),
    'far': dict(seed=7, mag=1.5, far=True),
}
FRAC_MARGIN = 1e-4      # frac(flow * flow_scale) stays this far from 0 and 1: floor() agrees in fp32 and fp64
THRESH_MARGIN = 1e-3    # the thresholds of mask_terms: no mask bit depends on fp32 rounding
KINK = 0.005            # photometric Charbonnier kink (beta = 255, eps = 1e-3): |255 (im1 - im2w)| below five eps
KINK_SHARE_CAP = 5e-4   # at most this share of the pixels may be excluded as kink pixels
LOSS_REL = 1e-5         # kernel-level loss tolerance (test_loss_kernels_vs_oracle)
GRAD_TOL = 2e-4         # gradient tolerance relative to the tensor's max (same test)
GRAY_W = (0.2989, 0.5870, 0.1140)


# the cases both the GPU tests and their CPU proof run
SMOOTH_CASES = [('RAGGED', 'm1.5'), ('XCD', 'm4.0'), ('ROW', 'm1.5'), ('TINY', 'm1.5'), ('BIG', 'm1.5'), ('BIG', 'm4.0')]
WARP_CASES = SMOOTH_CASES + [('RAGGED', 'far'), ('XCD', 'far'), ('BIG', 'far')]              # terms that warp an image
GRAY_CASES = [(n, k) for n, k in WARP_CASES if n in ('RAGGED', 'XCD', 'BIG')]
CENSUS_CASES = ([(n, k, D, m) for n, k in (('RAGGED', 'm1.5'), ('XCD', 'far')) for D in range(5) for m in (1, 'N')] +
                [('ROW', 'm1.5', 3, 1), ('ROW', 'm1.5', 3, 'N'), ('TINY', 'm1.5', 0, 1), ('TINY', 'm1.5', 0, 'N'),
                 ('BIG', 'm1.5', 1, 1), ('BIG', 'm4.0', 4, 'N')])                                 # (shape, set, D, n_mask)
MASK_CASES = ([(n, k, mode, nb) for n, k in SMOOTH_CASES[:4] for mode in (0, 1, 2) for nb in (0, 1, 'N')] +
              [('BIG', 'm1.5', 1, 0), ('BIG', 'm4.0', 2, 1), ('BIG', 'm1.5', 0, 'N')])            # (.., occlusion_mode, n_base; 0 = outgoing mask)
MASK_WEIGHTS = [(0.2, 0.0, 0.0), (0.0, 12.4, 0.0), (0.0, 0.0, 1.0), (0.2, 12.4, 1.0)]            # fb, occ, sym alone; all three


def n_of(code, name):
    """'N' in a case stands for the shape's batch."""
    return SHAPES[name][0] if code == 'N' else code


def flow_scale(name):
    return 1.0 if name == 'BIG' else 2.5


# ------------------------------------------------------------------------------------------------ inputs
def frac_margin(flow, fs):
    """Distance of frac(flow * fs) from {0, 1}, in fp64."""
    v = flow.double() * fs
    fr = v - v.floor()
    return torch.minimum(fr, 1 - fr)


def _draw_flow(g, shape, mag, far, fs):
    f = torch.randn(*shape, 2, generator=g) * mag
    if far:
        sel = torch.rand(*shape, generator=g) < 0.2
        n = int(sel.sum())
        sign = (torch.rand(n, 2, generator=g) < 0.5).float() * 2 - 1
        f[sel] = sign * 50.0 + torch.randn(n, 2, generator=g)
    for _ in range(64):
        bad = frac_margin(f, fs) < FRAC_MARGIN
        if not bad.any():
            return f
        f[bad] = torch.randn(int(bad.sum()), generator=g) * mag
    raise RuntimeError("flow margin not reached")


def _draw_mask(g, n, H, W):
    return (torch.rand(n, H, W, 1, generator=g) > 0.2).float() * torch.rand(n, H, W, 1, generator=g)


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """im [N,H,W,3] in [0,1], flow [N,H,W,2], masks [1,H,W,1] / [N,H,W,1], and the planes / warped image the kernels that do not
    warp themselves take as arguments (fp32 torch-CPU evaluations: any fp32 plane is a valid input)."""
    N, H, W = SHAPES[name]
    s = SETS[kind]
    fs = flow_scale(name)
    g = torch.Generator().manual_seed(s['seed'] * 1000 + H)
    im = torch.rand(N, H, W, 3, generator=g)
    flow = _draw_flow(g, (N, H, W), s['mag'], s['far'], fs)
    d = dict(name=name, kind=kind, N=N, B=N // 2, H=H, W=W, fs=fs, im=im, flow=flow,
             mask1=_draw_mask(g, 1, H, W), maskN=_draw_mask(g, N, H, W))
    im2w = M.image_warp(partner(im), flow * fs)
    d['im2w'] = im2w
    d['gray1'] = (M.rgb_to_grayscale(im) * 255)[..., 0].contiguous()
    d['gray2w'] = (M.rgb_to_grayscale(im2w) * 255)[..., 0].contiguous()
    return d


def partner(t):
    """t[(n + B) % N] for every n."""
    return torch.roll(t, shifts=-(t.shape[0] // 2), dims=0)


def _grid(H, W):
    return torch.arange(W, dtype=torch.float64).view(1, 1, W), torch.arange(H, dtype=torch.float64).view(1, H, 1)


def mask_margins(flow, warped, fwarp, fs):
    """The three margins of mask_terms in fp64, each [N,H,W]: |lhs - rhs| of the fb_occ inequality, |fwarp - 0.8|, and the
    distance of (x+u, y+v) from the image's edges 0 and W-1 / H-1."""
    N, H, W, _ = flow.shape
    u, w = flow.double() * fs, warped.double() * fs
    fb = (M.length_sq(u + w) - (0.01 * (M.length_sq(u) + M.length_sq(w)) + 0.5)).abs()[..., 0]
    gx, gy = _grid(H, W)
    px, py = gx + u[..., 0], gy + u[..., 1]
    edge = torch.stack([px.abs(), (px - (W - 1)).abs(), py.abs(), (py - (H - 1)).abs()]).amin(0)
    return fb, (fwarp.double() - M.DISOCC_THRESH).abs(), edge


@functools.lru_cache(maxsize=None)
def make_mask_inputs(name, kind):
    """The arguments of unflow_mask_terms built directly: flow, warped_other (about -flow: a forward-backward pair), fwarp
    (forward-warp densities around the 0.8 threshold) and base masks, with the threshold margins enforced by resampling."""
    N, H, W = SHAPES[name]
    s = SETS[kind]
    fs = flow_scale(name)
    g = torch.Generator().manual_seed(s['seed'] * 1000 + H + 500)
    flow = _draw_flow(g, (N, H, W), s['mag'], False, fs)
    warped = -flow + torch.randn(N, H, W, 2, generator=g) * 0.5
    fwarp = torch.rand(N, H, W, generator=g) * 2
    for _ in range(64):
        fb, dis, edge = mask_margins(flow, warped, fwarp, fs)
        b_edge, b_fb, b_dis = edge < THRESH_MARGIN, fb < THRESH_MARGIN, dis < THRESH_MARGIN
        if not (b_edge.any() or b_fb.any() or b_dis.any()):
            break
        if b_edge.any():
            flow[b_edge] = _draw_flow(g, (int(b_edge.sum()),), s['mag'], False, fs)
        bw = b_fb | b_edge
        warped[bw] = -flow[bw] + torch.randn(int(bw.sum()), 2, generator=g) * 0.5
        fwarp[b_dis] = torch.rand(int(b_dis.sum()), generator=g) * 2
    else:
        raise RuntimeError("mask margins not reached")
    return dict(name=name, kind=kind, N=N, B=N // 2, H=H, W=W, fs=fs, flow=flow, warped=warped, fwarp=fwarp,
                base1=_draw_mask(g, 1, H, W), baseN=_draw_mask(g, N, H, W))


# ------------------------------------------------------------------------------------------------ references
def _leaf(t, dt):
    return t.to(dt).clone().requires_grad_()


def _halves(fn, B, *ts):
    """The oracle's functions take one direction ([B,...]); a directed batch is the sum over both."""
    return fn(*[t[:B] for t in ts]) + fn(*[t[B:] for t in ts])


def _mask(inp, n_mask, dt, key='mask'):
    m = inp[key + ('1' if n_mask == 1 else 'N')].to(dt)
    return m.expand(inp['N'], inp['H'], inp['W'], 1)


@functools.lru_cache(maxsize=None)
def ref_smooth(term, name, kind, dt, weight=3.0):
    """term 'second_order' | 'smooth_1st': loss and d/d(flow)."""
    inp = make_inputs(name, kind)
    fn = M.second_order_loss if term == 'second_order' else M.smoothness_loss
    fl = _leaf(inp['flow'], dt)
    loss = weight * _halves(lambda f: fn(f * inp['fs']), inp['B'], fl)
    loss.backward()
    return dict(loss=loss.item(), d_flow=fl.grad)


@functools.lru_cache(maxsize=None)
def ref_photometric(name, kind, n_mask, dt, weight=1.5):
    """photometric_loss(im1 - image_warp(im2, flow*fs), mask): loss, d/d(flow) and (fp64 only meaningful) the kink pixels."""
    inp = make_inputs(name, kind)
    im = inp['im'].to(dt)
    fl = _leaf(inp['flow'], dt)
    diff = im - M.image_warp(partner(im), fl * inp['fs'])
    loss = weight * _halves(M.photometric_loss, inp['B'], diff, _mask(inp, n_mask, dt))
    loss.backward()
    kink = (255.0 * diff.detach()).abs().amin(3) < KINK
    return dict(loss=loss.item(), d_flow=fl.grad, kink=kink)


@functools.lru_cache(maxsize=None)
def ref_gradient(name, kind, n_mask, dt, weight=2.0):
    """gradient_loss(im1, im2w, mask) with the warped image as an argument: loss and d/d(im2w)."""
    inp = make_inputs(name, kind)
    w = _leaf(inp['im2w'], dt)
    loss = weight * _halves(M.gradient_loss, inp['B'], inp['im'].to(dt), w, _mask(inp, n_mask, dt))
    loss.backward()
    return dict(loss=loss.item(), d_im2w=w.grad)


@functools.lru_cache(maxsize=None)
def ref_gradient_chain(name, kind, n_mask, dt, weight=2.0):
    """gradient_loss(im1, image_warp(im2, flow*fs), mask): loss and d/d(flow), as the engine chains the kernels."""
    inp = make_inputs(name, kind)
    im = inp['im'].to(dt)
    fl = _leaf(inp['flow'], dt)
    loss = weight * _halves(M.gradient_loss, inp['B'], im, M.image_warp(partner(im), fl * inp['fs']), _mask(inp, n_mask, dt))
    loss.backward()
    return dict(loss=loss.item(), d_flow=fl.grad)


def gray_as_rgb(g):
    """An [.., 3] image whose rgb_to_grayscale(.) * 255 is the plane g (the census kernels take gray planes, the oracle's
    ternary_loss takes images): g / (255 * sum of the gray weights) in every channel."""
    return (g / (255.0 * sum(GRAY_W))).unsqueeze(-1).expand(*g.shape, 3)


@contextlib.contextmanager
def _capture_charbonnier_input():
    """The tensors handed to the oracle's charbonnier_loss (the census distance inside ternary_loss), kept with their
    gradients: d(loss)/d(dist) is what unflow_ternary_fwd leaves in dist_out."""
    seen, orig = [], M.charbonnier_loss

    def wrapped(x, *a, **k):
        x.retain_grad()
        seen.append(x)
        return orig(x, *a, **k)

    M.charbonnier_loss = wrapped
    try:
        yield seen
    finally:
        M.charbonnier_loss = orig


@functools.lru_cache(maxsize=None)
def ref_census(name, kind, D, n_mask, dt, weight=4.35):
    """ternary_loss on the gray planes: loss, d(loss)/d(dist) [N,H,W] and d/d(gray2w) [N,H,W]."""
    inp = make_inputs(name, kind)
    g1, g2 = inp['gray1'].to(dt), _leaf(inp['gray2w'], dt)
    with _capture_charbonnier_input() as seen:
        loss = weight * _halves(lambda a, b, m: M.ternary_loss(gray_as_rgb(a), gray_as_rgb(b), m, D), inp['B'],
                                g1, g2, _mask(inp, n_mask, dt))
        loss.backward()
    return dict(loss=loss.item(), d_dist=torch.cat([x.grad for x in seen])[..., 0], d_gray2w=g2.grad)


@functools.lru_cache(maxsize=None)
def ref_warp_gray(name, kind, dt):
    """gray(im) and gray(image_warp(im2, flow*fs)), both * 255."""
    inp = make_inputs(name, kind)
    im = inp['im'].to(dt)
    w = M.image_warp(partner(im), inp['flow'].to(dt) * inp['fs'])
    return dict(gray1=(M.rgb_to_grayscale(im) * 255)[..., 0], gray2w=(M.rgb_to_grayscale(w) * 255)[..., 0])


@functools.lru_cache(maxsize=None)
def ref_mask_terms(name, kind, mode, n_base, weights, dt):
    """The mask and the fb / occ / sym terms of compute_losses (losses.py:25-73) from the oracle's pieces.  mode 0 none, 1 'fb',
    2 'disocc'; n_base 0: create_outgoing_mask; weights = (fb, occ, sym).  Returns loss, mask [N,H,W], d/d(flow), d/d(warped)."""
    inp = make_mask_inputs(name, kind)
    fs, B = inp['fs'], inp['B']
    fl, wp = _leaf(inp['flow'], dt), _leaf(inp['warped'], dt)
    u, w = fl * fs, wp * fs
    mask = M.create_outgoing_mask(u.detach()) if n_base == 0 else _mask(inp, n_base, dt, 'base')
    fb_occ = (M.length_sq(u + w) > 0.01 * (M.length_sq(u) + M.length_sq(w)) + 0.5).to(dt).detach()
    dis = (partner(inp['fwarp'].to(dt)) < M.DISOCC_THRESH).to(dt).unsqueeze(3)
    if mode == 1:
        mask = mask * (1 - fb_occ)
    elif mode == 2:
        mask = mask * (1 - dis)
    occ = 1 - mask
    w_fb, w_occ, w_sym = weights
    loss = torch.zeros((), dtype=dt)
    if w_occ:
        loss = loss + w_occ * _halves(M.charbonnier_loss, B, occ)
    if w_sym:
        loss = loss + w_sym * _halves(M.charbonnier_loss, B, occ - dis)
    if w_fb:
        loss = loss + w_fb * _halves(M.charbonnier_loss, B, u + w, mask)
        loss.backward()
    zero = torch.zeros_like(fl)
    return dict(loss=loss.item(), mask=mask[..., 0].float().contiguous(), d_flow=fl.grad if w_fb else zero,
                d_warped=wp.grad if w_fb else zero)


# ------------------------------------------------------------------------------------------------ comparators
def check_loss(got, ref, rel=LOSS_REL):
    """|got - ref| <= rel * |ref|; returns the ratio."""
    got, ref = float(got), float(ref)
    ratio = abs(got - ref) / max(abs(ref), 1e-30)
    assert ratio <= rel, ("loss", got, ref, ratio, rel)
    return ratio


def max_rel(got, ref, exclude=None):
    """max |got - ref| / max |ref| over the elements outside `exclude` (a boolean mask over the leading pixel axes)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    if exclude is not None:
        ex = exclude.reshape(exclude.shape + (1,) * (err.dim() - exclude.dim())).expand_as(err)
        err = err.masked_fill(ex, 0.0)
    scale = ref.abs().max().item()
    if scale == 0.0:
        return 0.0 if err.max().item() == 0.0 else float('inf')
    return (err.max() / scale).item()      # NaN in `got` gives NaN, which fails every `<=`


def check_grad(got, ref, tol, exclude=None, max_share=KINK_SHARE_CAP):
    """Every element of got within tol * max|ref| of ref; returns the worst ratio.  `exclude`: pixels left out, whose share of all
    pixels this comparator caps at max_share."""
    if exclude is not None:
        share = int(exclude.sum()) / exclude.numel()
        assert share <= max_share, ("excluded share", share, max_share)
    worst = max_rel(got, ref, exclude)
    assert worst <= tol, ("gradient", worst, tol)
    return worst


def check_mask(got, ref):
    """Bit for bit."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    n = int((got != ref).sum())
    assert n == 0, ("mask pixels differ", n)


def grad_bound(ref32, ref64, exclude=None, floor=GRAD_TOL):
    """max(floor, 2 x the fp32 torch-CPU oracle's own max-rel error against fp64 on the same inputs): the kernels use the ~1 ulp
    hardware rsq / rcp / exp / log forms where the CPU rounds correctly.  Returns (bound, the oracle's error)."""
    own = max_rel(ref32, ref64, exclude)
    return max(floor, 2.0 * own), own
