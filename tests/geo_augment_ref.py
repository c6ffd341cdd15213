"""Inputs, the reference and the comparators of the geometric-augmentation tests (tests/test_geo_augment_gpu.py, proven without a
GPU by tests/test_geo_augment_cpu.py).  Not a test file.

`evaluate` is the definition of unflow_supervised_geo_augment (include/unflow_hip.h) in numpy: evaluated in fp64
it is THE reference, in fp32 — the same expression order as the kernel — the yardstick of what fp32 arithmetic can deliver.
Both run on the same fp32-rounded matrices and inputs.

Margin.  A pixel is excluded when a coordinate that feeds a floor() lies within MARGIN = 1e-3 of an integer in fp64: s1.x, s1.y
(image 1 and mode 0), s1 + 0.5 (mode 1), s2 (image 2).  fp32 coordinates at W ~ 800 carry ~1e-4 px of rounding, so 1e-3 is
safe.  One refinement, which only ever excludes FEWER pixels: a coordinate whose fp32 and fp64 evaluations are exactly equal is
not excluded — both sides floor the same number.  That is the case of the 'identity' and 'flips' sets below, whose maps are
exact whole-pixel maps (every coordinate an integer, every product exact): all their pixels are compared.  (Their theta
counterparts, theta = I and a theta flip, are slight zooms, x = px W / (W - 1): they put whole border rows and columns on
integers, 15 % of a 19 x 45 image, and the pixels there would all be excluded; the transformer's theta path is covered by the
'full' set, the im1-against-transformer test and the engine tests.)
Cap.  The excluded share is at most CAP = 2 % of the pixels of a case (expectation 4 * 1e-3 = 0.4 %).
Tolerance.  Outside the margin the mask is bit-exact and flow / images agree within max(2 x the yardstick's own worst error
against fp64, 2^-20 (H + W)) — the floor is about eight roundings of a coordinate of size H + W (for the images: times a slope
of at most one grey range per pixel)."""
import functools

import numpy as np
import torch

MARGIN = 1e-3
CAP = 0.02
SHAPES = [(4, 19, 45), (3, 37, 47), (2, 7, 70), (2, 333, 795)]     # the last: 529,470 px, past stream_grid's 2048 x 256
SETS = ('identity', 'flips', 'full')
MODES = (0, 1)
CASES = [(s, k) for s in SHAPES for k in SETS]
HOLE_SHARE = 0.03
FULL_RANGES = dict(max_translation_x=0.1, max_translation_y=0.1, max_rotation=10.0, min_scale=0.9, max_scale=1.1)
SEEDS = {'identity': 11, 'flips': 12, 'full': 13}


def coord_floor(H, W):
    return 2.0 ** -20 * (H + W)


# ------------------------------------------------------------------------------------------------ inputs
def smooth_images(B, H, W, seed):
    """Two smooth [B,H,W,3] fp32 image batches in [0,255]."""
    g = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = []
    for _ in range(2):
        ph = g.uniform(0, 6.28, size=(B, 1, 1, 3))
        im = 127.5 + 100.0 * np.sin(x[None, :, :, None] / 12.0 + ph) * np.cos(y[None, :, :, None] / 9.0 + 0.5 * ph)
        out.append(im.astype(np.float32))
    return out


def noisy_gt(B, H, W, seed, holes=True):
    """flow [B,H,W,2] = randn * 4, mask [B,H,W,1] with HOLE_SHARE holes; under the holes the flow is 1e10 or NaN (what the
    Chairs / Middlebury readers keep there)."""
    g = np.random.RandomState(seed + 1000)
    flow = (g.randn(B, H, W, 2) * 4.0).astype(np.float32)
    mask = np.ones((B, H, W, 1), dtype=np.float32)
    if holes:
        hole = g.rand(B, H, W) < HOLE_SHARE
        mask[hole] = 0.0
        junk = np.where(g.rand(B, H, W) < 0.5, np.float32(1e10), np.float32(np.nan)).astype(np.float32)
        flow[hole] = junk[hole][:, None]
    return flow, mask


def whole_pixel_mats(B, H, W, flip=None, dx=None, dy=None):
    """Exact whole-pixel maps [B,3,6] fp32: x' = x + dx (or W - 1 - x + dx where flip), y' = y + dy, the same for M1 and M2,
    with the exact inverse."""
    flip = np.zeros(B, bool) if flip is None else np.asarray(flip, bool)
    dx = np.zeros(B) if dx is None else np.asarray(dx, np.float64)
    dy = np.zeros(B) if dy is None else np.asarray(dy, np.float64)
    m = np.zeros((B, 3, 6), dtype=np.float64)
    for b in range(B):
        a = -1.0 if flip[b] else 1.0
        c = (W - 1.0 if flip[b] else 0.0) + dx[b]
        fwd = [a, 0.0, c, 0.0, 1.0, dy[b]]
        inv = [a, 0.0, -a * c, 0.0, 1.0, -dy[b]]           # x = a (x' - c)
        m[b] = [fwd, fwd, inv]
    return m.astype(np.float32)


def draw_mats(B, H, W, kind, seed):
    """The [B,3,6] fp32 maps of a draw set."""
    from unflow_amd.core import augment as A
    if kind == 'identity':
        return whole_pixel_mats(B, H, W)
    if kind == 'flips':
        return whole_pixel_mats(B, H, W, flip=[b % 2 == 0 for b in range(B)])
    g = torch.Generator().manual_seed(seed)
    tg = A.draw_affine(B, horizontal_flipping=True, generator=g, **FULL_RANGES)
    tl = A.draw_affine(B, generator=g, **FULL_RANGES)
    return A.affine_pixel_maps(tg, tl, H, W).numpy()


@functools.lru_cache(maxsize=None)
def case_inputs(shape, kind):
    B, H, W = shape
    seed = SEEDS[kind] + 7 * H
    im1, im2 = smooth_images(B, H, W, seed)
    flow, mask = noisy_gt(B, H, W, seed)
    return dict(im1=im1, im2=im2, flow=flow, mask=mask, mats=draw_mats(B, H, W, kind, seed))


def photometric_draws(B, seed):
    from unflow_amd.core import augment as A
    return A.draw_supervised_augmentation(B, torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the definition
def _apply(m, k, x, y):
    r = m[:, k]
    c = lambda j: r[:, j, None, None]
    return (c(0) * x + c(1) * y) + c(2), (c(3) * x + c(4) * y) + c(5)


def _image_taps(im, x, y):
    """stn_affine_kernel's tap rule on taps v / 255: floor, indices clipped before the weights, its add order."""
    B, H, W, _ = im.shape
    dt = x.dtype
    fx = np.minimum(np.maximum(np.floor(x), dt.type(-4)), dt.type(W + 4))
    fy = np.minimum(np.maximum(np.floor(y), dt.type(-4)), dt.type(H + 4))
    x0, x1 = np.clip(fx.astype(np.int64), 0, W - 1), np.clip(fx.astype(np.int64) + 1, 0, W - 1)
    y0, y1 = np.clip(fy.astype(np.int64), 0, H - 1), np.clip(fy.astype(np.int64) + 1, 0, H - 1)
    x0f, x1f, y0f, y1f = (a.astype(dt) for a in (x0, x1, y0, y1))
    wa, wb = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f)
    wc, wd = (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
    n = np.arange(B)[:, None, None]
    s = im / dt.type(255.0)
    pa, pb, pc, pd = s[n, y0, x0], s[n, y1, x0], s[n, y0, x1], s[n, y1, x1]
    e = lambda w: w[..., None]
    return ((e(wa) * pa + e(wb) * pb) + e(wc) * pc) + e(wd) * pd


def evaluate(im1, im2, flow, mask, mats, mode, dtype):
    """The kernel's definition in `dtype` arithmetic.  Returns im01 [2B,H,W,3], flow [B,H,W,2], mask [B,H,W,1] and the
    coordinates s1, s2 [B,H,W] x 2."""
    dt = np.dtype(dtype)
    B, H, W, _ = im1.shape
    m = np.asarray(mats).astype(dt)
    im1, im2, flow = (np.asarray(a).astype(dt) for a in (im1, im2, flow))
    mk = np.ones((B, H, W), dt) if mask is None else np.asarray(mask).astype(dt).reshape(B, H, W)
    py, px = np.meshgrid(np.arange(H).astype(dt), np.arange(W).astype(dt), indexing='ij')
    px, py = px[None], py[None]
    s1x, s1y = _apply(m, 0, px, py)
    s2x, s2y = _apply(m, 1, px, py)
    im01 = np.concatenate([_image_taps(im1, s1x, s1y), _image_taps(im2, s2x, s2y)], 0)
    n = np.arange(B)[:, None, None]
    with np.errstate(invalid='ignore', over='ignore'):
        if mode == 0:
            fx, fy = np.floor(s1x), np.floor(s1y)
            inside = (fx >= 0) & (fx + 1 <= W - 1) & (fy >= 0) & (fy + 1 <= H - 1)
            xi, yi = np.clip(fx.astype(np.int64), 0, W - 2), np.clip(fy.astype(np.int64), 0, H - 2)
            valid = inside & (mk[n, yi, xi] > 0.5) & (mk[n, yi, xi + 1] > 0.5) & (mk[n, yi + 1, xi] > 0.5) & (mk[n, yi + 1, xi + 1] > 0.5)
            ax, ay = (s1x - fx)[..., None], (s1y - fy)[..., None]
            t00, t01, t10, t11 = flow[n, yi, xi], flow[n, yi, xi + 1], flow[n, yi + 1, xi], flow[n, yi + 1, xi + 1]
            r0, r1 = t00 + (t01 - t00) * ax, t10 + (t11 - t10) * ax
            f = r0 + (r1 - r0) * ay
        else:
            rx, ry = np.floor(s1x + dt.type(0.5)), np.floor(s1y + dt.type(0.5))
            inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
            xi, yi = np.clip(rx.astype(np.int64), 0, W - 1), np.clip(ry.astype(np.int64), 0, H - 1)
            valid = inside & (mk[n, yi, xi] > 0.5)
            f = flow[n, yi, xi]
        f = np.where(valid[..., None], f, dt.type(0))
        qx, qy = _apply(m, 2, s1x + f[..., 0], s1y + f[..., 1])
        out = np.stack([qx - px, qy - py], -1)
    out = np.where(valid[..., None], out, dt.type(0))
    return dict(im01=im01, flow=out, mask=valid.astype(dt)[..., None], s1=(s1x, s1y), s2=(s2x, s2y))


# ------------------------------------------------------------------------------------------------ comparators
def _near_integer(c64, c32):
    d = np.abs(c64 - np.round(c64)) < MARGIN
    return d & (c64 != c32.astype(np.float64))          # equal in both precisions: both floor the same number


def excluded(ref, yard, mode):
    """(gt, im1, im2) boolean [B,H,W]: the pixels the margin rule leaves out of the ground-truth, image-1 and image-2
    comparisons."""
    near = lambda k, j, off=0.0: _near_integer(ref[k][j] + off, yard[k][j] + np.float32(off))
    e1 = near('s1', 0) | near('s1', 1)
    e2 = near('s2', 0) | near('s2', 1)
    gt = e1 if mode == 0 else (near('s1', 0, 0.5) | near('s1', 1, 0.5))
    return gt, e1, e2


class Reference:
    """Reference (fp64), yardstick (fp32), exclusions and bounds of one case and mode — computed once."""

    def __init__(self, inputs, mode):
        a = inputs
        self.mode = mode
        B, H, W, _ = a['im1'].shape
        self.B, self.H, self.W = B, H, W
        self.ref = evaluate(a['im1'], a['im2'], a['flow'], a['mask'], a['mats'], mode, np.float64)
        self.yard = evaluate(a['im1'], a['im2'], a['flow'], a['mask'], a['mats'], mode, np.float32)
        self.ex_gt, self.ex_im1, self.ex_im2 = excluded(self.ref, self.yard, mode)
        self.ex_im = np.concatenate([self.ex_im1, self.ex_im2], 0)
        self.shares = dict(gt=self.ex_gt.mean(), im1=self.ex_im1.mean(), im2=self.ex_im2.mean())
        self.yard_flow_err = self.flow_err(self.yard['flow'])
        self.yard_im_err = self.image_err(self.yard['im01'])
        self.flow_tol = max(2.0 * self.yard_flow_err, coord_floor(H, W))
        self.im_tol = max(2.0 * self.yard_im_err, coord_floor(H, W))

    def flow_err(self, flow):
        d = np.abs(np.asarray(flow, np.float64) - self.ref['flow']).max(-1)
        return float(d[~self.ex_gt].max())

    def image_err(self, im01):
        d = np.abs(np.asarray(im01, np.float64) - self.ref['im01']).max(-1)
        return float(d[~self.ex_im].max())

    def mask_mismatches(self, mask):
        m = np.asarray(mask, np.float64).reshape(self.B, self.H, self.W)
        return int(((m != self.ref['mask'][..., 0]) & ~self.ex_gt).sum())


@functools.lru_cache(maxsize=None)
def reference(shape, kind, mode):
    return Reference(case_inputs(shape, kind), mode)


# ------------------------------------------------------------------------------------------------ warp consistency
WARP_SHAPES = [(2, 37, 47), (1, 128, 192)]
WARP_TOL = 0.5          # grey levels: bilinear error of im1 <= (|dxx| + |dyy|) / 8 ~ 0.33 plus the flow's interpolation error ~ 0.03


def _I2(x, y):
    return 127.5 + 100.0 * np.sin(x / 12.0) * np.cos(y / 9.0)


def _flow_field(x, y):
    return 4 * np.sin(x / 25.0) + 2 * np.cos(y / 20.0), 3 * np.cos(x / 30.0) - 2 * np.sin(y / 18.0)


@functools.lru_cache(maxsize=None)
def warp_inputs(shape):
    """im1(s) = I2(s + f(s)) on the pixel grid with a smooth flow f: the second frame is I2 itself, so the augmented first
    frame at p must equal I2 at M2 (p + flow'(p)) wherever flow' is valid — whatever the formula behind flow' is."""
    B, H, W = shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    fu, fv = _flow_field(x, y)
    im1 = _I2(x + fu, y + fv)
    rep = lambda a: np.repeat(np.repeat(a[None, :, :, None], B, 0), 3, 3).astype(np.float32)
    flow = np.repeat(np.stack([fu, fv], -1)[None], B, 0).astype(np.float32)
    return dict(im1=rep(im1), im2=rep(_I2(x, y)), flow=flow, mask=np.ones((B, H, W, 1), np.float32),
                mats=draw_mats(B, H, W, 'full', 21 + H))


def warp_consistency_error(im01, flow, mask, mats):
    """max |255 im1_geo(p) - I2(M2 (p + flow'(p)))| over the valid pixels, and the number of valid pixels."""
    B = flow.shape[0]
    H, W = flow.shape[1:3]
    m = np.asarray(mats, np.float64)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    fl = np.asarray(flow, np.float64)
    tx, ty = _apply(m, 1, x[None] + fl[..., 0], y[None] + fl[..., 1])
    want = _I2(tx, ty)
    got = 255.0 * np.asarray(im01, np.float64)[:B, :, :, 0]
    valid = np.asarray(mask).reshape(B, H, W) > 0.5
    return float(np.abs(got - want)[valid].max()), int(valid.sum())
