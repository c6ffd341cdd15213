"""Cases, inputs, exact fp64 values and bounds of the tests that pin the oracle and the HIP ops to the reference's own GPU kernels
(tests/test_reference_kernels_gpu.py; the conditions are checked without a GPU in tests/test_reference_build_cpu.py).

Every compared output element is a sum of n products.  `exact` functions return, per element and in fp64, the value v of that
sum, S = sum |terms| (the final division included) and n.  ANY fp32 evaluation of the sum, in any order, with or without fused
multiply-adds, lies within

    gamma = (n + 2) * 2^-24 * S

of v: n - 1 additions and one rounding per product leave at most n * u * S to first order (u = 2^-24), the final division one
more u, and the last unit of slack covers the second-order terms for the n <= 10^4 of these cases.  Two fp32 sides are therefore
within 2 * gamma of each other.  Nothing here is measured from the code under test.

What keeps the bound honest (checked by test_reference_build_cpu.py):
  * flows are dyadic — multiples of 1/16, |flow| < 32 — so float(x) + u is exact in fp32, every floorf() picks the same cell in
    every implementation, the bilinear weights (multiples of 1/16) and their pairwise products (multiples of 1/256) are exact,
    and the splat's exponent -(dx^2 + dy^2) / 2 is exact.  No element has to be excluded: the allowed share is zero;
  * values on integers, zero flows and flows that leave the image are part of every field.
"""
import functools
import math
import zlib

import numpy as np

U = 2.0 ** -24

# N, C, H, W, kernel_size, max_displacement, pad, stride_1, stride_2
CORR_CASES = [
    (2, 32, 9, 11, 1, 3, 5, 1, 1),        # 49 channels: pad > displacement, ragged
    (2, 64, 12, 40, 1, 4, 4, 1, 1),       # 81: the +-4 cost volume
    (2, 96, 16, 24, 1, 20, 20, 1, 2),     # 441: FlowNetC's displacement grid and its channel ordering
    (2, 40, 7, 30, 1, 10, 10, 1, 1),      # 441 at stride_2 = 1
    (2, 16, 10, 13, 3, 4, 5, 2, 2),       # kernel_size 3, stride_1 2
    (2, 33, 6, 9, 1, 2, 2, 1, 1),         # C not a multiple of the 32 reference lanes
]
CORR_IDS = ["49ch_pad5_md3", "81ch", "441ch_s2", "441ch_s1", "k3_s1_2", "C33"]
ONE_HOT_CASE = 2

WARP_SIZES = [(2, 9, 13), (1, 17, 6)]
WARP_CHANNELS = [1, 3]
DOWNSAMPLE_SCALES = [2, 4]                # tests/test_ops_gpu.py::test_downsample_vs_oracle
DOWNSAMPLE_SHAPES = [(2, 8, 12, 3), (1, 16, 4, 1)]


def attrs_of(case):
    return dict(kernel_size=case[4], max_displacement=case[5], pad=case[6], stride_1=case[7], stride_2=case[8])


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def gamma(n, S):
    return (np.asarray(n, np.float64) + 2.0) * U * S


# ------------------------------------------------------------------------------------------------ correlation
def corr_geometry(H, W, k, md, pad, s1, s2):
    """oc, oh, ow, r, gw, ph, pw: border = md + (k - 1) / 2 on each side of the PADDED image, output every s1 pixels."""
    kr = (k - 1) // 2
    r = md // s2
    gw = 2 * r + 1
    ph, pw = H + 2 * pad, W + 2 * pad
    oh = -(-(ph - 2 * (md + kr)) // s1)
    ow = -(-(pw - 2 * (md + kr)) // s1)
    return gw * gw, oh, ow, r, gw, ph, pw


@functools.lru_cache(maxsize=None)
def corr_inputs(idx):
    """in0, in1 (independent draws, NCHW fp32) and dout."""
    N, C, H, W, k, md, pad, s1, s2 = CORR_CASES[idx]
    rs = _rs("corr", idx)
    oc, oh, ow = corr_geometry(H, W, k, md, pad, s1, s2)[:3]
    return _ro(rs.randn(N, C, H, W).astype(np.float32), rs.randn(N, C, H, W).astype(np.float32),
               rs.randn(N, oc, oh, ow).astype(np.float32))


@functools.lru_cache(maxsize=None)
def corr_one_hot_inputs():
    """One non-zero pixel in each input of the 441-channel case: in0 at (y, x), in1 at (y + dy, x + dx) with dy != dx, unequal
    values.  Exactly one output element is non-zero; which channel says how the displacement grid is ordered."""
    N, C, H, W = CORR_CASES[ONE_HOT_CASE][:4]
    a, b = np.zeros((N, C, H, W), np.float32), np.zeros((N, C, H, W), np.float32)
    a[1, 5, 7, 9] = 2.0
    b[1, 5, 7 - 6, 9 + 8] = 3.0
    return _ro(a, b)


def _padded(x, pad):
    return np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)))


def corr_exact_fwd(in0, in1, k, md, pad, s1, s2):
    """(v, S, n) of the cost volume, NCHW."""
    N, C, H, W = in0.shape
    oc, oh, ow, r, gw, ph, pw = corr_geometry(H, W, k, md, pad, s1, s2)
    P0, P1 = _padded(in0, pad), _padded(in1, pad)
    v, S = np.zeros((N, oc, oh, ow)), np.zeros((N, oc, oh, ow))
    for ch in range(oc):
        dy, dx = (ch // gw - r) * s2, (ch % gw - r) * s2
        for j in range(k):
            for i in range(k):
                y0, x0 = md + j, md + i
                a = P0[:, :, y0:y0 + (oh - 1) * s1 + 1:s1, x0:x0 + (ow - 1) * s1 + 1:s1]
                b = P1[:, :, y0 + dy:y0 + dy + (oh - 1) * s1 + 1:s1, x0 + dx:x0 + dx + (ow - 1) * s1 + 1:s1]
                t = a * b
                v[:, ch] += t.sum(1)
                S[:, ch] += np.abs(t).sum(1)
    return v / (k * k * C), S / (k * k * C), k * k * C


def corr_exact_bwd(dout, in0, in1, k, md, pad, s1, s2):
    """((v0, S0, n0), (v1, S1, n1)) of the two input gradients, NCHW: the adjoint of corr_exact_fwd written out as a scatter over
    (channel, patch tap, output site); n counts the sites x channels x taps that reach an input pixel."""
    N, C, H, W = in0.shape
    oc, oh, ow, r, gw, ph, pw = corr_geometry(H, W, k, md, pad, s1, s2)
    P0, P1 = _padded(in0, pad), _padded(in1, pad)
    d64 = dout.astype(np.float64)
    G = [np.zeros_like(P0) for _ in range(4)]                    # v0, S0, v1, S1
    cnt = [np.zeros((ph, pw)), np.zeros((ph, pw))]
    for ch in range(oc):
        dy, dx = (ch // gw - r) * s2, (ch % gw - r) * s2
        d = d64[:, ch][:, None]
        for j in range(k):
            for i in range(k):
                y0, x0 = md + j, md + i
                s0 = (slice(None), slice(None), slice(y0, y0 + (oh - 1) * s1 + 1, s1), slice(x0, x0 + (ow - 1) * s1 + 1, s1))
                s1_ = (slice(None), slice(None), slice(y0 + dy, y0 + dy + (oh - 1) * s1 + 1, s1),
                       slice(x0 + dx, x0 + dx + (ow - 1) * s1 + 1, s1))
                t0, t1 = d * P1[s1_], d * P0[s0]
                G[0][s0] += t0
                G[1][s0] += np.abs(t0)
                G[2][s1_] += t1
                G[3][s1_] += np.abs(t1)
                cnt[0][s0[2:]] += 1
                cnt[1][s1_[2:]] += 1
    crop = (slice(None), slice(None), slice(pad, pad + H), slice(pad, pad + W))
    den = k * k * C
    n0 = np.broadcast_to(cnt[0][crop[2:]], (N, C, H, W))
    n1 = np.broadcast_to(cnt[1][crop[2:]], (N, C, H, W))
    return (G[0][crop] / den, G[1][crop] / den, n0), (G[2][crop] / den, G[3][crop] / den, n1)


@functools.lru_cache(maxsize=None)
def corr_exact(idx):
    """{'out' | 'grad0' | 'grad1': (v, S, n)} of a case, computed once."""
    in0, in1, dout = corr_inputs(idx)
    a = CORR_CASES[idx][4:]
    g0, g1 = corr_exact_bwd(dout, in0, in1, *a)
    return {"out": corr_exact_fwd(in0, in1, *a), "grad0": g0, "grad1": g1}


# ------------------------------------------------------------------------------------------------ flows
def dyadic_flow(rs, B, H, W):
    """[B,H,W,2] fp32, every value a multiple of 1/16 with |value| < 32: mostly within +-4 pixels, a sixth anywhere in +-32 (most
    of those leave these small images), a sixth on integers, one row of exact zeros."""
    f = rs.randint(-64, 65, size=(B, H, W, 2)).astype(np.float64)
    far = rs.rand(B, H, W) < 1.0 / 6
    f[far] = rs.randint(-511, 512, size=(int(far.sum()), 2))
    whole = rs.rand(B, H, W) < 1.0 / 6
    f[whole] = np.round(f[whole] / 16.0) * 16.0
    f[:, H // 2] = 0.0
    f = np.clip(f, -511, 511) / 16.0
    return f.astype(np.float32)


def flow_conditions(flow):
    """The conditions of the module docstring on a flow field: dyadic, bounded, x + u exact in fp32, and integers, zeros and
    out-of-image targets present."""
    B, H, W, _ = flow.shape
    f64 = flow.astype(np.float64)
    assert np.array_equal(f64 * 16, np.round(f64 * 16)) and np.abs(f64).max() < 32
    gx, gy = np.meshgrid(np.arange(W), np.arange(H))
    for c, grid in ((0, gx), (1, gy)):
        t32 = grid.astype(np.float32)[None] + flow[..., c]                      # the implementations' fp32 sum
        assert np.array_equal(t32.astype(np.float64), grid[None] + f64[..., c])  # is the exact sum
    tx, ty = gx[None] + f64[..., 0], gy[None] + f64[..., 1]
    assert np.any((f64 == np.round(f64)) & (f64 != 0)) and np.any(f64 == 0)
    assert np.any((tx < -1) | (tx > W) | (ty < -1) | (ty > H))
    assert np.any((f64 != np.round(f64)))


@functools.lru_cache(maxsize=None)
def warp_inputs(size, C):
    """im [B,H,W,C], flow [B,H,W,2], dout [B,H,W,C] (fp32)."""
    B, H, W = size
    rs = _rs("warp", size, C)
    return _ro(rs.randn(B, H, W, C).astype(np.float32), dyadic_flow(rs, B, H, W), rs.randn(B, H, W, C).astype(np.float32))


# ------------------------------------------------------------------------------------------------ backward_warp
def bw_exact(im, flow, dout):
    """{'out': (v, S, n) [B,H,W,C], 'd_flow': (v, S, n) [B,H,W,2]}: bilinear taps at floor(x + u), out-of-image taps dropped;
    d_flow sums, over channels and taps, -/+ (row weight) * I * dout for u and -/+ (column weight) * I * dout for v."""
    B, H, W, C = im.shape
    I, D, F = im.astype(np.float64), dout.astype(np.float64), flow.astype(np.float64)
    out = [np.zeros((B, H, W, C)) for _ in range(2)]
    dfl = [np.zeros((B, H, W, 2)) for _ in range(2)]
    n_out, n_dfl = np.zeros((B, H, W, C)), np.zeros((B, H, W, 2))
    for b in range(B):
        for y in range(H):
            for x in range(W):
                sx, sy = x + F[b, y, x, 0], y + F[b, y, x, 1]
                x0, y0 = math.floor(sx), math.floor(sy)
                wr, wb = sx - x0, sy - y0
                wl, wt = 1.0 - wr, 1.0 - wb
                for (tx, ty, wx, wy, sgx, sgy) in ((x0, y0, wl, wt, -1, -1), (x0 + 1, y0, wr, wt, 1, -1),
                                                   (x0, y0 + 1, wl, wb, -1, 1), (x0 + 1, y0 + 1, wr, wb, 1, 1)):
                    if not (0 <= tx < W and 0 <= ty < H):
                        continue
                    t = wx * wy * I[b, ty, tx]
                    out[0][b, y, x] += t
                    out[1][b, y, x] += np.abs(t)
                    n_out[b, y, x] += 1
                    q = I[b, ty, tx] * D[b, y, x]
                    dfl[0][b, y, x, 0] += (sgx * wy * q).sum()
                    dfl[0][b, y, x, 1] += (sgy * wx * q).sum()
                    dfl[1][b, y, x, 0] += np.abs(wy * q).sum()
                    dfl[1][b, y, x, 1] += np.abs(wx * q).sum()
                    n_dfl[b, y, x] += C
    return {"out": (out[0], out[1], n_out), "d_flow": (dfl[0], dfl[1], n_dfl)}


# ------------------------------------------------------------------------------------------------ forward_warp
def fw_exact(flow, dout):
    """{'out': (v, S, n) [B,H,W,1], 'd_flow': (v, S, n) [B,H,W,2]}: every source splats exp(-(dx^2 + dy^2) / 2) onto the integer
    sites from floor(t - 4) to floor(t + 4), clipped to the image, unless that square misses the image; d_flow gathers
    dout * weight * (dx, dy) over the same sites.  n: contributions that land on the element."""
    B, H, W, _ = flow.shape
    F, D = flow.astype(np.float64), dout.astype(np.float64).reshape(B, H, W)
    out, n_out = np.zeros((B, H, W)), np.zeros((B, H, W))
    dfl = [np.zeros((B, H, W, 2)) for _ in range(2)]
    n_dfl = np.zeros((B, H, W, 2))
    for b in range(B):
        for y in range(H):
            for x in range(W):
                tx, ty = x + F[b, y, x, 0], y + F[b, y, x, 1]
                if not (math.floor(tx - 4) < W and math.floor(tx + 4) >= 0 and math.floor(ty - 4) < H and math.floor(ty + 4) >= 0):
                    continue
                xs = np.arange(math.floor(tx - 4) if tx - 4 > 0 else 0, (math.floor(tx + 4) if tx + 4 < W else W - 1) + 1)
                ys = np.arange(math.floor(ty - 4) if ty - 4 > 0 else 0, (math.floor(ty + 4) if ty + 4 < H else H - 1) + 1)
                dx, dy = np.meshgrid(xs - tx, ys - ty)
                w = np.exp(-(dx * dx + dy * dy) / 2.0)
                sl = (b, slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
                out[sl] += w
                n_out[sl] += 1
                t = D[sl] * w
                dfl[0][b, y, x] = ((t * dx).sum(), (t * dy).sum())
                dfl[1][b, y, x] = (np.abs(t * dx).sum(), np.abs(t * dy).sum())
                n_dfl[b, y, x] = w.size
    return {"out": (out[..., None], out[..., None].copy(), n_out[..., None]), "d_flow": (dfl[0], dfl[1], n_dfl)}


# ------------------------------------------------------------------------------------------------ downsample
@functools.lru_cache(maxsize=None)
def ds_inputs(shape):
    return _ro(_rs("downsample", shape).randn(*shape).astype(np.float32))


def ds_exact(im, scale):
    B, H, W, C = im.shape
    x = im.astype(np.float64).reshape(B, H // scale, scale, W // scale, scale, C)
    return x.mean(axis=(2, 4)), np.abs(x).mean(axis=(2, 4)), scale * scale


@functools.lru_cache(maxsize=None)
def warp_exact(size, C):
    im, flow, dout = warp_inputs(size, C)
    return {"backward_warp": bw_exact(im, flow, dout), "forward_warp": fw_exact(flow, dout[..., :1])}


# ------------------------------------------------------------------------------------------------ comparison
def ratio_to_bound(a, b, bound):
    """max over the elements of |a - b| / bound; where the bound is 0 (an empty or all-zero sum) the two must be equal, else inf.
    NaN anywhere is inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), a.shape)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b)
    if not np.all(np.isfinite(err)):
        return float("inf")
    zero = bound == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def assert_within(what, got, exact, factor=1.0, other=None):
    """|got - v| <= factor * gamma per element (other given: |got - other| <= factor * gamma).  Prints and returns the ratio."""
    v, S, n = exact
    ratio = ratio_to_bound(got, v if other is None else other, factor * gamma(n, S))
    print("REFPIN %-64s worst |diff| / bound = %.4f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio
