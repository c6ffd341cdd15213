"""fp64 numpy mirror of the flow visualisation (csrc/visual.hip), written from its definitions: the colour wheel, the KITTI
error image, overlay / brightness error and the 8-bit conversion.  Inputs are taken as given (float32 arrays are widened, never
re-rounded); every operation is fp64.  The colour-map constants are the float32 values rgb / 255 that an fp32 image holds (the
reference forms its map in np.float32): a mirror with fp64 constants would describe an image no fp32 pipeline can produce, and
would put every halved odd level (243 / 2 = 121.5) on a rounding tie."""
import numpy as np

COLORMAP = [(0, 0.0625, 49, 54, 149), (0.0625, 0.125, 69, 117, 180), (0.125, 0.25, 116, 173, 209), (0.25, 0.5, 171, 217, 233),
            (0.5, 1, 224, 243, 248), (1, 2, 254, 224, 144), (2, 4, 253, 174, 97), (4, 8, 244, 109, 67), (8, 16, 215, 48, 39),
            (16, 1000000000.0, 165, 0, 38)]
EDGES = [c[0] for c in COLORMAP[1:]]                    # the inner bin edges 0.0625 .. 16


def to_bytes(img):
    """byte = floor(min(max(x * 255, 0), 255) + 0.5)."""
    return np.floor(np.clip(np.asarray(img, np.float64) * 255.0, 0.0, 255.0) + 0.5).astype(np.uint8)


def ref_angle(u, v):
    """The reference's atan2 table: u == 0 gives +-pi, u == v == 0 gives 0 here (NaN there; the pixel is white anyway)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        at = np.arctan(v / u)
    a = np.zeros_like(u)
    a = np.where(u > 0, at, a)
    a = np.where((u < 0) & (v >= 0), at + np.pi, a)
    a = np.where((u < 0) & (v < 0), at - np.pi, a)
    a = np.where((u == 0) & (v > 0), np.pi, a)
    a = np.where((u == 0) & (v < 0), -np.pi, a)
    return a


def flow_to_color(flow, mask=None, max_flow=None):
    """flow [..., 2], mask [...] or [..., 1] -> [..., 3] in [0, 1].  max_flow None: max |flow * mask| over the whole array."""
    flow = np.asarray(flow, np.float64)
    m = np.ones(flow.shape[:-1]) if mask is None else np.asarray(mask, np.float64).reshape(flow.shape[:-1])
    u, v = flow[..., 0], flow[..., 1]
    mf = max(float(max_flow), 1.0) if max_flow is not None else float(np.max(np.abs(flow * m[..., None]), initial=0.0))
    mag = np.sqrt(u * u + v * v)
    hue = np.mod(ref_angle(u, v) / (2 * np.pi) + 1.0, 1.0)
    s = np.clip(mag * 8 / mf, 0, 1) if mf > 0 else np.zeros_like(mag)
    d = 6 * hue
    rgb = np.stack([np.clip(np.abs(d - 3) - 1, 0, 1), np.clip(2 - np.abs(d - 2), 0, 1), np.clip(2 - np.abs(d - 4), 0, 1)], -1)
    return ((1 - s)[..., None] + s[..., None] * rgb) * m[..., None]


def kitti_error(flow_1, flow_2):
    """min(diff / 3, 20 diff / |gt|) in fp64 (|gt| == 0: diff / 3)."""
    f1, f2 = np.asarray(flow_1, np.float64), np.asarray(flow_2, np.float64)
    diff = np.sqrt(((f1 - f2) ** 2).sum(-1))
    mag = np.sqrt((f2 ** 2).sum(-1))
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(mag > 0, 20 * diff / mag, np.inf)
    return np.minimum(diff / 3, rel), diff


def flow_error_image(flow_1, flow_2, mask_occ, mask_noc=None, log_colors=True):
    error, diff = kitti_error(flow_1, flow_2)
    mo = np.asarray(mask_occ, np.float64).reshape(error.shape)
    mn = np.ones_like(mo) if mask_noc is None else np.asarray(mask_noc, np.float64).reshape(error.shape)
    if not log_colors:
        e = np.minimum(diff, 5) / 5 * mo
        return np.stack([e, e * mn, e * mn], -1)
    im = np.zeros(error.shape + (3,))
    for lo, hi, r, g, b in COLORMAP:
        col = (np.array([r, g, b], np.float32) / np.float32(255)).astype(np.float64)
        im = np.where(((error >= lo) & (error < hi))[..., None], col, im)
    im = np.where((mn != 0)[..., None], im, im * 0.5)
    return im * mo[..., None]


def edge_band(error, rel=1e-4):
    """Pixels whose error lies within a relative `rel` of a bin edge: fp32 evaluation may put them in the neighbouring bin."""
    error = np.asarray(error, np.float64)
    near = np.zeros(error.shape, bool)
    for e in EDGES:
        near |= np.abs(error - e) <= rel * e
    return near


def resize_tf1(x, oh, ow):
    """TF1 legacy bilinear resize of [H, W, C] (align_corners=False): src = dst * in / out, the scale an fp32 quotient and the
    source coordinate an fp32 product as in csrc/resize_tf1.h (they choose the taps); the interpolation in fp64."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[:2]
    fy = (np.arange(oh, dtype=np.float32) * (np.float32(H) / np.float32(oh))).astype(np.float32)
    fx = (np.arange(ow, dtype=np.float32) * (np.float32(W) / np.float32(ow))).astype(np.float32)
    y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly, lx = (fy.astype(np.float64) - y0)[:, None, None], (fx.astype(np.float64) - x0)[None, :, None]
    top = x[y0][:, x0] + (x[y0][:, x1] - x[y0][:, x0]) * lx
    bot = x[y1][:, x0] + (x[y1][:, x1] - x[y1][:, x0]) * lx
    return top + (bot - top) * ly


def image_warp(im, flow):
    """image_warp.py: bilinear taps at (x, y) + flow, indices x + floor(u) clamped to the image; flow float32 [h, w, 2]."""
    im = np.asarray(im, np.float64)
    h, w = im.shape[:2]
    fl = np.asarray(flow, np.float64)
    fu, fv = np.floor(fl[..., 0]), np.floor(fl[..., 1])
    xw, yw = (fl[..., 0] - fu)[..., None], (fl[..., 1] - fv)[..., None]
    yy, xx = np.mgrid[0:h, 0:w]
    big = 1 << 40                                         # vectors far outside the image: clamp before the integer cast
    xi, yi = xx + np.clip(fu, -big, big).astype(np.int64), yy + np.clip(fv, -big, big).astype(np.int64)
    x0, x1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    y0, y1 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    return (1 - xw) * (1 - yw) * im[y0, x0] + (1 - xw) * yw * im[y1, x0] + xw * (1 - yw) * im[y0, x1] + xw * yw * im[y1, x1]


def shown_frame(frame, H, W):
    """The frame the reference shows: resize_input to the network size, resize_output back."""
    h, w = np.asarray(frame).shape[:2]
    return resize_tf1(resize_tf1(frame, H, W), h, w)


def overlay_and_diff(frame1, frame2, flow, H, W):
    im1, im2 = shown_frame(frame1, H, W), shown_frame(frame2, H, W)
    return (0.5 * im1 + 0.5 * im2) / 255.0, np.abs(im1 - image_warp(im2, flow)) / 255.0
