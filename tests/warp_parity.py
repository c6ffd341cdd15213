"""Cases, inputs, fp64 mirrors and comparators of the per-pixel parity tests of csrc/ops_warp.hip (tests/test_warp_kernels_gpu.py,
proven without a GPU by tests/test_warp_parity_cpu.py).  Not a test file.

forward_warp and backward_warp are mirrored in numpy from the reference's definition (ops/forward_warp_op.cu.cc:16-125,
ops/backward_warp_op.cu.cc:27-67), not from the kernels: the fp32 sums and floorf() of the reference CHOOSE the taps (they are
part of the definition: which pixels a source reaches), everything after that — distances, weights, sums — is fp64.  The fp32
C oracle (oracle/ops_ref.c) is the yardstick of what fp32 arithmetic delivers on the same inputs: the standing bound is
max(floor, 2 x the oracle's own distance from the mirror) of the tensor's max.  image_warp is the fp64 autograd of the oracle's
own function, as in tests/loss_parity.py."""
import functools
import math

import numpy as np
import torch

import loss_parity as LP
from oracle import model_ref as M

FLOOR = 1e-6                    # the bound's floor, of the tensor's max
FRAC_MARGIN = LP.FRAC_MARGIN    # gradient comparisons of the two bilinear warps leave out pixels this close to a tap switch ...
EXCLUDE_CAP = 1e-3              # ... and at most this share of them
REJECT = 1e6                    # a flow that throws its source out of every image here

# ------------------------------------------------------------------------------------------------ forward_warp: cases
# name -> (B, H, W): the smallest shapes that reach each path (source tiles 64 x 16, LDS window 104 x 56, target tiles 32 x 32,
# grid caps 2048 source tiles / 4096 target tiles, one scan workgroup of 1024 threads)
FW_SHAPES = {
    'TINY': (2, 2, 3),          # footprints clipped on all four sides; narrower than a footprint
    'NINE': (2, 9, 9),          # x_hi - x_lo == 8 only for a centred source: the 9 x 9 fast branch beside the clipped one
    'NINE2': (2, 10, 8),        # ... and an image one short / one over
    'RAGGED': (3, 19, 45),      # partial source tiles only: 45 of 64 columns, 16 and 3 of 16 rows
    'WINDOW': (2, 70, 130),     # larger than the window; ragged against source and target tiles
    'TILECAP': (2050, 3, 5),    # 2050 source tiles: the tile kernel's second grid-stride pass
    'BINCAP': (700, 4, 200),    # 2800 source tiles, 4900 target tiles: second pass of fill and gather, 5 bins per scan thread
    'TENTH': (1, 24, 40),       # constructed: three live sources with ten-wide / ten-tall footprints, the rest rejected
    'TENTHFAR': (1, 40, 136),   # constructed: two such sources of one source tile, too far apart for its window (the binned gather takes them)
}
FW_KINDS = ('m1.5', 'm4.0', 'far', 'torn', 'tiny')
FW_CASES = [('TINY', 'm1.5'), ('TINY', 'tiny'), ('NINE', 'm1.5'), ('NINE2', 'm1.5'), ('NINE', 'tiny'),
            ('RAGGED', 'm1.5'), ('RAGGED', 'm4.0'), ('RAGGED', 'far'), ('RAGGED', 'tiny'),
            ('WINDOW', 'm4.0'), ('WINDOW', 'far'), ('WINDOW', 'torn'),
            ('TILECAP', 'm1.5'), ('BINCAP', 'm1.5'), ('BINCAP', 'torn'),
            ('TENTH', 'built'), ('TENTHFAR', 'built')]
FW_BWD_FORMS_CASES = [('RAGGED', 'm4.0'), ('WINDOW', 'far'), ('TENTH', 'built'), ('TENTHFAR', 'built')]   # rows and dword gradient kernels
TORN_CASES = [('WINDOW', 'torn'), ('BINCAP', 'torn')]
# (tx, ty) of the live sources, as decimal strings of fp32 numbers, and the pixel each one starts from; expected ranges
TENTH_SOURCES = {
    'TENTH': [((10, 8), (12.999999, 8.5), (8, 17, 4, 12)),              # ten wide
              ((20, 14), (20.5, 12.999999), (16, 24, 8, 17)),           # ten tall
              ((30, 3), (28.999998, 4.9999995), (24, 33, 0, 9))],       # both; the row range starts at the clipped 0
    'TENTHFAR': [((9, 2), (12.999999, 4.9999995), (8, 17, 0, 9)),           # both in the source tile (0, 0) ...
                 ((60, 10), (124.99999, 28.999998), (120, 129, 24, 33))],   # ... this one across the target-tile seams x = 128, y = 32
}
TINY_VALUES = (-1e-8, 1e-8, -1.0 + 1e-8, 0.99999994)     # the `tiny` set of tests/test_ops_gpu.py::_flows


def _rs(*key):
    import zlib
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def draw_flow(rs, B, H, W, kind, torn_u_only=False):
    """[B,H,W,2] fp32 of one of the flow sets."""
    if kind in ('m1.5', 'm4.0', 'far'):
        f = rs.randn(B, H, W, 2) * (4.0 if kind == 'm4.0' else 1.5)
        if kind == 'far':
            sel = rs.rand(B, H, W) < 0.2
            n = int(sel.sum())
            f[sel] = rs.choice([-50.0, 50.0], size=(n, 2)) + rs.randn(n, 2)
    elif kind == 'torn':                                    # uniform +-60 px
        f = rs.rand(B, H, W, 2) * 120 - 60
        if torn_u_only:
            f[..., 1] = rs.randn(B, H, W) * 1.5
    elif kind == 'tiny':
        f = rs.choice(TINY_VALUES, size=(B, H, W, 2))
    else:
        raise ValueError(kind)
    return f.astype(np.float32)


def _blocks(n):
    """Flat pixel ranges of the block of exact zeros and of the block of rejected sources."""
    k = max(1, n // 16)
    return (n // 8, n // 8 + k), (n // 2, n // 2 + k)


@functools.lru_cache(maxsize=None)
def fw_inputs(name, kind):
    """flow [B,H,W,2] and dout [B,H,W] (fp32 numpy, read-only).  Every drawn set carries a block of exact zeros and a block of
    rejected sources (+-1e6, every third of them inf, every fourth NaN)."""
    B, H, W = FW_SHAPES[name]
    rs = _rs('fw', name, kind)
    if kind == 'built':
        flow = np.full((B, H, W, 2), REJECT, np.float32)
        flow[:, ::2, :, 0] = -REJECT
        for (px, py), (tx, ty), _ in TENTH_SOURCES[name]:
            flow[0, py, px] = (np.float32(tx) - np.float32(px), np.float32(ty) - np.float32(py))
    else:
        flow = draw_flow(rs, B, H, W, kind, torn_u_only=(name == 'BINCAP'))
        flat = flow.reshape(-1, 2)
        (z0, z1), (r0, r1) = _blocks(B * H * W)
        flat[z0:z1] = 0.0
        rej = rs.choice([-REJECT, REJECT], size=(r1 - r0, 2)).astype(np.float32)
        rej[::3, 0] = np.inf
        rej[1::3, 1] = -np.inf
        rej[::4, rs.randint(2)] = np.nan
        flat[r0:r1] = rej
    dout = rs.randn(B, H, W).astype(np.float32)
    flow.setflags(write=False)
    dout.setflags(write=False)
    return dict(name=name, kind=kind, B=B, H=H, W=W, flow=flow, dout=dout)


# ------------------------------------------------------------------------------------------------ forward_warp: fp64 mirror
def fw_footprints(flow, bounds64=False, clip_w=False, splat_rejected=False):
    """forward_warp_op.cu.cc:29-30, 46-51: tx = fl32(px + u); the accept test and the four bounds are fp32 floorf() of fp32 sums.
    Returns ok [B,H,W] bool, tx, ty (fp32) and lo / hi per axis (int64; 0 / -1 where rejected: an empty range).
    Mutants: bounds64 — bounds from the fp64 sum; clip_w — hi clipped to W, not W - 1; splat_rejected — a rejected source is
    clamped into the image and splatted."""
    B, H, W, _ = flow.shape
    k = np.float32(4.0)                                     # ceilf(2 + 2)
    px = np.arange(W, dtype=np.float32).reshape(1, 1, W)
    py = np.arange(H, dtype=np.float32).reshape(1, H, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        tx = (px + flow[..., 0]).astype(np.float32)
        ty = (py + flow[..., 1]).astype(np.float32)
        assert tx.dtype == np.float32 and (tx - k).dtype == np.float32
        ok = (np.floor(tx - k) < W) & (np.floor(tx + k) >= 0) & (np.floor(ty - k) < H) & (np.floor(ty + k) >= 0)
        if splat_rejected:
            tx = np.where(ok, tx, np.clip(np.nan_to_num(tx, nan=0.0), 0, W - 1)).astype(np.float32)
            ty = np.where(ok, ty, np.clip(np.nan_to_num(ty, nan=0.0), 0, H - 1)).astype(np.float32)
            ok = np.ones_like(ok)
        sx, sy, kk = (tx.astype(np.float64), ty.astype(np.float64), 4.0) if bounds64 else (tx, ty, k)
        z = np.zeros_like(sx)

        def rng(s, size):
            lo = np.where(ok & (s - kk > 0), np.floor(np.where(ok, s - kk, z)), 0)
            hi = np.where(s + kk < size, np.floor(np.where(ok, s + kk, z)), size if clip_w else size - 1)
            return lo.astype(np.int64), np.where(ok, hi, -1).astype(np.int64)
        x_lo, x_hi = rng(sx, W)
        y_lo, y_hi = rng(sy, H)
    return dict(ok=ok, tx=tx, ty=ty, x_lo=np.where(ok, x_lo, 0), x_hi=x_hi, y_lo=np.where(ok, y_lo, 0), y_hi=y_hi)


def fw_ranges(fp):
    """What unflow_forward_warp_ranges reports: {x_lo, x_hi, y_lo, y_hi}, all -1 where rejected."""
    r = np.stack([fp['x_lo'], fp['x_hi'], fp['y_lo'], fp['y_hi']], axis=-1)
    return np.where(fp['ok'][..., None], r, -1).astype(np.int32)


def fw_mirror(flow, dout=None, cap=10, strict_hi=False, divisor=2.0, grad_no_dx=False, seam=False, **foot):
    """The reference's splat and its gradient in fp64 over the reference's own taps: dx = nx - tx with tx widened,
    exp(-(dx^2 + dy^2) / 2), np.bincount sums.  Returns (out [B,H,W], d_flow [B,H,W,2] or None, footprints).
    Mutants: cap — at most this many taps per axis (9: the nine-tap kernels); strict_hi — n < hi; divisor — exp(-d^2 / 4);
    grad_no_dx — d_flow without the factor dx; seam — a tap at x = 0 mod 32 is dropped unless it is its source's first column
    (a tile seam that loses one column); and the footprint mutants of fw_footprints."""
    B, H, W, _ = flow.shape
    n = B * H * W
    fp = fw_footprints(flow, **foot)
    src = np.flatnonzero(fp['ok'].reshape(-1))
    b = src // (H * W)
    g = {key: fp[key].reshape(-1)[src] for key in ('x_lo', 'x_hi', 'y_lo', 'y_hi')}
    tx, ty = fp['tx'].reshape(-1)[src].astype(np.float64), fp['ty'].reshape(-1)[src].astype(np.float64)
    out = np.zeros(n)
    du, dv = np.zeros(n), np.zeros(n)
    d = None if dout is None else dout.astype(np.float64).reshape(-1)
    for i in range(cap):
        ny = g['y_lo'] + i
        my = ny < g['y_hi'] if strict_hi else ny <= g['y_hi']
        if not my.any():
            continue
        for j in range(cap):
            nx = g['x_lo'] + j
            m = my & (nx < g['x_hi'] if strict_hi else nx <= g['x_hi'])
            if seam:
                m &= ~((nx % 32 == 0) & (j > 0))
            idx = (b[m] * H + ny[m]) * W + nx[m]            # (clip_w: x = W runs into the next row ...)
            inside = idx < n                                # (... or past the tensor's end: dropped)
            if not inside.all():
                m[np.flatnonzero(m)[~inside]] = False
                idx = idx[inside]
            if idx.size == 0:
                continue
            dx, dy = nx[m] - tx[m], ny[m] - ty[m]
            w = np.exp(-(dx * dx + dy * dy) / divisor)
            out += np.bincount(idx, weights=w, minlength=n)
            if d is not None:
                factor = 2.0 * d[idx] * w / divisor         # :115
                du += np.bincount(src[m], weights=factor if grad_no_dx else factor * dx, minlength=n)
                dv += np.bincount(src[m], weights=factor * dy, minlength=n)
    d_flow = None if d is None else np.stack([du, dv], axis=-1).reshape(B, H, W, 2)
    return out.reshape(B, H, W), d_flow, fp


@functools.lru_cache(maxsize=None)
def fw_ref(name, kind):
    """The mirror of a case and the fp32 C oracle on the same inputs, computed once: out / d_flow (fp64 torch), ranges (int32
    numpy), o_out / o_d_flow / o_ranges (the oracle's), far_share / far_tiles (far_share())."""
    from oracle import ops_ref
    inp = fw_inputs(name, kind)
    out, d_flow, fp = fw_mirror(inp['flow'], inp['dout'])
    share, tiles = far_share(fp)
    r = dict(out=torch.from_numpy(out), d_flow=torch.from_numpy(d_flow), ranges=fw_ranges(fp), ok=fp['ok'],
             far_share=share, far_tiles=tiles)
    r['o_out'] = torch.from_numpy(ops_ref.forward_warp(inp['flow'])[..., 0].copy())
    r['o_d_flow'] = torch.from_numpy(ops_ref.forward_warp_grad(inp['dout'][..., None], inp['flow']))
    r['o_ranges'] = ops_ref.forward_warp_ranges(inp['flow'])
    return r


def far_share(fp, tx=64, ty=16, wx=104, wy=56):
    """(share, source tiles with such a source per image [B]): share of the accepted sources whose footprint does not lie inside their source tile's window as a whole.  The window of
    a 64 x 16 source tile is 104 x 56 target pixels centred on the mean footprint centre of the tile's accepted sources
    (integer means, as the scatter kernel forms them) — counted from the mirror's footprints."""
    ok = fp['ok']
    B, H, W = ok.shape
    far = total = 0
    tiles = np.zeros(B, dtype=np.int64)
    for y0 in range(0, H, ty):
        for x0 in range(0, W, tx):
            sl = (slice(None), slice(y0, y0 + ty), slice(x0, x0 + tx))
            o = ok[sl]
            cnt = o.sum(axis=(1, 2))
            xl, xh, yl, yh = (fp[key][sl] for key in ('x_lo', 'x_hi', 'y_lo', 'y_hi'))
            safe = np.maximum(cnt, 1) * 2
            wx0 = ((xl + xh) * o).sum(axis=(1, 2)) // safe - wx // 2
            wy0 = ((yl + yh) * o).sum(axis=(1, 2)) // safe - wy // 2
            wx0, wy0 = wx0.reshape(B, 1, 1), wy0.reshape(B, 1, 1)
            inside = (xl >= wx0) & (xh < wx0 + wx) & (yl >= wy0) & (yh < wy0 + wy)
            far += int((o & ~inside).sum())
            tiles += (o & ~inside).any(axis=(1, 2))
            total += int(o.sum())
    return far / max(total, 1), tiles


@functools.lru_cache(maxsize=None)
def fw_border_case():
    """The constructed gradient case (3 x 20 x 37): every source rejected except (a) one whose footprint is clipped at the right
    border, with NaN in dout at the start of the rows that follow its footprint rows — the columns a 36-byte row load brings in
    and must drop; (b) one in the last rows of the last image (rows past y_hi: the out-of-range row offset); (c) one in the
    last image's bottom right corner, whose last row load runs past the tensor's end.  dout is finite on every tap of the
    three footprints."""
    B, H, W = 3, 20, 37
    flow = np.full((B, H, W, 2), -REJECT, np.float32)
    flow[0, 6, 33] = (1.25, 0.5)           # tx = 34.25: columns 30..36, clipped at W - 1 = 36
    flow[2, 18, 20] = (-2.5, 0.75)         # ty = 18.75: rows 14..19, the image's and the tensor's last
    flow[2, 18, 34] = (0.25, 0.75)         # both
    rs = _rs('fw_border')
    dout = rs.randn(B, H, W).astype(np.float32)
    dout[:, :, 0:2] = np.nan               # what follows column 36 of the row above in memory
    fp = fw_footprints(flow)
    assert fw_ranges(fp)[0, 6, 33].tolist() == [30, 36, 2, 10] and fw_ranges(fp)[2, 18, 20].tolist() == [13, 21, 14, 19]
    assert fw_ranges(fp)[2, 18, 34].tolist() == [30, 36, 14, 19] and int(fp['ok'].sum()) == 3
    safe = np.nan_to_num(dout, nan=0.0)    # the mirror reads no NaN: columns 0..1 are outside every footprint
    _, d_flow, _ = fw_mirror(flow, safe)
    from oracle import ops_ref
    o = ops_ref.forward_warp_grad(safe[..., None], flow)
    return dict(B=B, H=H, W=W, flow=flow, dout=dout, d_flow=torch.from_numpy(d_flow), o_d_flow=torch.from_numpy(o), ok=fp['ok'])


# ------------------------------------------------------------------------------------------------ backward_warp
BW_SHAPES = {'RAGGED': FW_SHAPES['RAGGED'], 'COLUMN': (2, 7, 1)}      # W = 1: the right tap is never in range
BW_CASES = [(s, k, C) for s in ('RAGGED', 'COLUMN') for k in ('m4.0', 'far', 'tiny') for C in (2, 5)]


def bw_frac_exclude(flow):
    """Pixels whose fp64 px + u or py + v lies within FRAC_MARGIN of an integer: the taps (chosen in fp32) switch there."""
    B, H, W, _ = flow.shape
    sx = np.arange(W, dtype=np.float64).reshape(1, 1, W) + flow[..., 0].astype(np.float64)
    sy = np.arange(H, dtype=np.float64).reshape(1, H, 1) + flow[..., 1].astype(np.float64)
    fr = np.stack([sx - np.floor(sx), sy - np.floor(sy)])
    return (np.minimum(fr, 1 - fr) < FRAC_MARGIN).any(axis=0)


@functools.lru_cache(maxsize=None)
def bw_inputs(shape, kind, C):
    """im [B,H,W,C], flow, dout (fp32 numpy) and the excluded pixels; redrawn until the exclusion keeps its cap (the `tiny` set
    sits on the tap switches by construction and is compared in values and indices only)."""
    B, H, W = BW_SHAPES[shape]
    for attempt in range(64):
        rs = _rs('bw', shape, kind, C, attempt)
        flow = draw_flow(rs, B, H, W, kind)
        ex = bw_frac_exclude(flow)
        if kind == 'tiny' or ex.mean() <= EXCLUDE_CAP:
            break
    else:
        raise RuntimeError("exclusion cap not reached")
    im = rs.rand(B, H, W, C).astype(np.float32)
    dout = rs.randn(B, H, W, C).astype(np.float32)
    return dict(B=B, H=H, W=W, C=C, kind=kind, im=im, flow=flow, dout=dout, exclude=torch.from_numpy(ex))


def bw_mirror(im, flow, dout=None, right_tap_at_edge=False):
    """backward_warp_op.cu.cc:27-67 and its gradient (:107-132) in fp64, the taps chosen in fp32: sx = fl32(px + u),
    x0 = floorf(sx); weights from the widened sx; taps outside the image are dropped.  Returns (out, d_flow or None, xy0 int32).
    Mutant: right_tap_at_edge — the right tap counts at x0 = W - 1 too (it reads the next row's first pixel)."""
    B, H, W, C = im.shape
    sx = (np.arange(W, dtype=np.float32).reshape(1, 1, W) + flow[..., 0]).astype(np.float32)
    sy = (np.arange(H, dtype=np.float32).reshape(1, H, 1) + flow[..., 1]).astype(np.float32)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    sx, sy = sx.astype(np.float64), sy.astype(np.float64)
    wr, wl, wb, wt = sx - x0, (x0 + 1) - sx, sy - y0, (y0 + 1) - sy
    flat = np.concatenate([im.astype(np.float64).reshape(-1, C), np.zeros((1, C))])     # (one row past the end: all zero)
    base = (np.arange(B) * H * W).reshape(B, 1, 1)
    out = np.zeros((B, H, W, C))
    du, dv = np.zeros((B, H, W)), np.zeros((B, H, W))
    d = None if dout is None else dout.astype(np.float64)
    for ox, oy, wx, wy, sgx, sgy in ((0, 0, wl, wt, -1, -1), (1, 0, wr, wt, 1, -1), (0, 1, wl, wb, -1, 1), (1, 1, wr, wb, 1, 1)):
        x, y = x0 + ox, y0 + oy
        x_in = (x >= 0) & ((x <= W) if (right_tap_at_edge and ox) else (x < W))
        m = x_in & (y >= 0) & (y < H)
        idx = np.where(m, np.minimum(base + y * W + x, B * H * W), B * H * W)
        v = flat[idx] * m[..., None]
        out += (wx * wy)[..., None] * v
        if d is not None:
            q = (v * d).sum(axis=-1)
            du += sgx * wy * q
            dv += sgy * wx * q
    d_flow = None if d is None else np.stack([du, dv], axis=-1)
    return out, d_flow, np.stack([x0, y0], axis=-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def bw_ref(shape, kind, C):
    from oracle import ops_ref
    inp = bw_inputs(shape, kind, C)
    out, d_flow, xy0 = bw_mirror(inp['im'], inp['flow'], inp['dout'])
    return dict(out=torch.from_numpy(out), d_flow=torch.from_numpy(d_flow), xy0=xy0,
                o_out=torch.from_numpy(ops_ref.backward_warp(inp['im'], inp['flow'])),
                o_d_flow=torch.from_numpy(ops_ref.backward_warp_grad(inp['dout'], inp['im'], inp['flow'])),
                o_xy0=ops_ref.backward_warp_indices(inp['flow']))


# ------------------------------------------------------------------------------------------------ image_warp
IW_SHAPE = FW_SHAPES['RAGGED']
IW_FS = 2.5
IW_CASES = [(k, C, shift) for k in ('m4.0', 'far', 'tiny') for C in (1, 5) for shift in (0, 1)]


@functools.lru_cache(maxsize=None)
def iw_inputs(kind, C):
    """im, flow, dout as fp32 torch.  frac(flow * fs) keeps FRAC_MARGIN from 0 and 1 (redrawn, tests/loss_parity.py), so the
    exclusion is empty; the `tiny` set is used at fs = 1 and compared in values and indices only."""
    B, H, W = IW_SHAPE
    g = torch.Generator().manual_seed(4100 + C + 10 * len(kind) + (7 if kind == 'far' else 0))
    if kind == 'tiny':
        flow = torch.from_numpy(draw_flow(_rs('iw', kind, C), B, H, W, kind))
        fs = 1.0
    else:
        flow = LP._draw_flow(g, (B, H, W), 4.0 if kind == 'm4.0' else 1.5, kind == 'far', IW_FS)
        fs = IW_FS
    im = torch.rand(B, H, W, C, generator=g)
    dout = torch.randn(B, H, W, C, generator=g)
    ex = (LP.frac_margin(flow, fs) < FRAC_MARGIN).any(3)
    return dict(B=B, H=H, W=W, C=C, kind=kind, fs=fs, im=im, flow=flow, dout=dout, exclude=ex)


@functools.lru_cache(maxsize=None)
def iw_ref(kind, C, shift, dt):
    """image_warp(im[(b + shift) % B], flow * fs) by the oracle's function in dtype dt, with autograd: out, d_im, d_flow."""
    inp = iw_inputs(kind, C)
    im, fl = inp['im'].to(dt).clone().requires_grad_(), inp['flow'].to(dt).clone().requires_grad_()
    out = M.image_warp(torch.roll(im, shifts=-shift, dims=0), fl * inp['fs'])
    out.backward(inp['dout'].to(dt))
    return dict(out=out.detach(), d_im=im.grad, d_flow=fl.grad)


def iw_indices(kind, C, shift):
    """The four gather indices (a, b, c, d) per pixel, relative to the batch, of the shifted source image: int32 [B,H,W,4]."""
    inp = iw_inputs(kind, C)
    B, H, W = inp['B'], inp['H'], inp['W']
    f = (inp['flow'] * np.float32(inp['fs'])).numpy() if inp['fs'] != 1.0 else inp['flow'].numpy()
    assert f.dtype == np.float32
    q = np.floor(f).astype(np.int64)
    px, py = np.arange(W).reshape(1, 1, W), np.arange(H).reshape(1, H, 1)
    x0, x1 = np.clip(px + q[..., 0], 0, W - 1), np.clip(px + q[..., 0] + 1, 0, W - 1)
    y0, y1 = np.clip(py + q[..., 1], 0, H - 1), np.clip(py + q[..., 1] + 1, 0, H - 1)
    base = (((np.arange(B) + shift) % B) * H * W).reshape(B, 1, 1)
    return np.stack([base + y0 * W + x0, base + y1 * W + x0, base + y0 * W + x1, base + y1 * W + x1], axis=-1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ downsample / resize_area
DS_GENERIC_CASES = [(1, 2), (2, 4), (5, 2), (3, 3), (3, 8), (4, 1)]      # (C, scale) that take downsample_kernel
DS_BIG = (2, 2 * 300, 2 * 450, 2, 2)                                     # B, H, W, C, scale: 540,000 outputs > 2048 * 256
RA_SIZES = [((5, 5), (2, 2)), ((7, 7), (3, 3)), ((3, 3), (7, 7)), ((37, 53), (18, 26)), ((1, 1), (1, 1))]
RA_BIG = (2, (310, 420), (300, 300), 3)                                  # 540,000 outputs, a fractional ratio on both axes


def ds_image(B, H, W, C, seed=0):
    return _rs('ds', B, H, W, C, seed).rand(B, H, W, C).astype(np.float32)


def area_weights(n_in, n_out):
    """[n_out, n_in] weights of tf.image.resize_area along one axis (TF's ResizeAreaOp): output i averages the source interval
    [i*s, (i+1)*s), s = n_in / n_out, every source pixel weighted by the covered fraction — the independent restatement.
    When upsampling the interval lies inside one pixel, or straddles two."""
    s = n_in / n_out
    w = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        lo, hi = i * s, (i + 1) * s
        for j in range(int(math.floor(lo)), min(n_in, int(math.ceil(hi)))):
            w[i, j] = (min(hi, j + 1) - max(lo, j)) / s
    return w


def resize_area_ref(t, oh, ow, dt=torch.float64):
    """tf.image.resize_area of an NHWC tensor from the separable area weights, in dtype dt."""
    B, H, W, C = t.shape
    return torch.einsum('yh,bhwc,xw->byxc', area_weights(H, oh).to(dt), t.to(dt), area_weights(W, ow).to(dt))


# ------------------------------------------------------------------------------------------------ comparators
def bound_of(oracle, mirror, exclude=None, floor=FLOOR):
    """(bound, the oracle's own ratio): max(floor, 2 x the fp32 oracle's distance from the fp64 mirror), of the tensor's max."""
    return LP.grad_bound(oracle, mirror, exclude, floor)


def check(got, mirror, bound, exclude=None):
    """Every element of got within bound * max|mirror| of the mirror; NaN fails; returns the worst ratio."""
    return LP.check_grad(got, mirror, bound, exclude, max_share=EXCLUDE_CAP)


def check_ranges(got, ref):
    """Bit for bit (int32)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    bad = int((got != ref).sum())
    assert bad == 0, ("integers differ", bad)


def check_rejected_zero(d_flow, ok):
    """The gradient of a rejected source is exactly (0, 0) (+0 or -0, no NaN)."""
    r = d_flow.detach().cpu()[~torch.as_tensor(ok)]
    assert bool((r == 0).all()), ("rejected sources with a gradient", int((r != 0).sum()))


def worst_pixel(got, mirror):
    """(index, got, mirror) of the element furthest from the mirror."""
    got, mirror = got.detach().cpu().double(), mirror.double()
    i = int((got - mirror).abs().nan_to_num(nan=float('inf')).argmax())
    idx = np.unravel_index(i, tuple(mirror.shape))
    return tuple(int(v) for v in idx), got.reshape(-1)[i].item(), mirror.reshape(-1)[i].item()
