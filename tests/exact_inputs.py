"""Inputs whose exact result is an fp32 number, for bit-exact tests of the bf16 x 3 (and fp16) matrix-core kernels.

The kernels split every operand into three bf16 planes (hi + mid + lo == x) and sum six plane products with fp32 accumulation.
On random data a lost term, tap or K slice is a 1e-6 wobble that the max-norm tolerances cannot see.  Here the operands are chosen
so that every plane product is exact AND every partial sum — in any order, under any split of K — is an fp32 number: the kernel
must then equal the fp64 reference bit for bit, and whatever it loses becomes a mismatch.

Regimes (operand a = activation side, operand b = weight side; `kinds` below):
  'A3'    a = +-(h +- 2^-9 +- 2^-18), h in {1, 1.25, 1.5, 1.75}: three non-zero planes; b in {-1, 0, +1}: hi plane only.
          The products are hi*hi, mid*hi, lo*hi: exposes the terms that read a's mid and lo planes.
  'B3'    the roles swapped: exposes hi*mid and hi*lo.
  'two'   both operands +-(h +- 2^-9), h in {1, 1.25}: two non-zero planes each; exposes mid*mid (2^-18).  (h stops at 1.25 so that
          four products stay inside the condition below: (1.25 + 2^-9)^2 * 4 < 8.)
  'dense' a in {-2 .. 2}, b in {-1, 0, 1}, nothing sparse: every (tap, channel, site) contributes to every output; exposes lost
          taps, K tails, tile tails, split-K slices and parity classes.
  'f16'   (n_planes == 1) a = +-(1 + n 2^-10), fp16-exact 11-bit significands; b in {-1, 0, +1}.

Condition (assert_condition, checked on the CPU by every test): with granule g = the smallest set bit of any product term (2^-18
in 'A3' / 'B3' / 'two', 2^-10 in 'f16', 1 in 'dense') every output satisfies sum_k |a_k b_k| + |bias| <= 2^21 g.  Every partial sum
is then a multiple of g below 2^21 g: 21 significant bits, three below fp32's 24.  In the 2^-18 regimes that is sum <= 8: about four
non-zero products per output, so one operand is sparse — few non-zeros per output, placed on the edges (first and last tap, the last
channel, the last site row and column, the last output column).  This is a condition on the generator, not a measurement of any
kernel.

MFMA exactness: the condition stands at 2^21 g — v_mfma_f32_32x32x16_bf16 / _f16 on the MI355X sum such products exactly (the
three-plane regimes are bit-exact on every kernel path of tests/test_exact_terms_gpu.py); it was not shrunk to 2^19 g.

emulated_gemm is the CPU model of the kernels' arithmetic (split, six terms, fp32 accumulation per term and K tile of 32) that
tests/test_exact_inputs_cpu.py uses to prove the regimes have teeth: any single term, tap or K tile removed is a mismatch."""
import torch
import torch.nn.functional as F

G3 = 2.0 ** -18
G16 = 2.0 ** -10
HEADROOM = 2.0 ** 21
GRANULE = {'A3': G3, 'B3': G3, 'two': G3, 'dense': 1.0, 'f16': G16}
REGIMES3 = ('A3', 'B3', 'two', 'dense')
REGIMES1 = ('f16', 'dense')
# the plane-product schedule of the kernels (planes_shared.h mfma_terms): (plane of a, plane of b), smallest terms first
TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
# the terms each regime is built to expose
EXPOSES = {'A3': ((2, 0), (1, 0)), 'B3': ((0, 2), (0, 1)), 'two': ((1, 1),)}


def gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ the split, emulated
def split3(x):
    """The library's split (igemm_shared.h split3): round-to-nearest-even bf16 at every level; three fp32 tensors."""
    x = x.float()
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    return hi, mid, lo


def emulated_gemm(a, b, drop=(), drop_rows=None, n_planes=3, ktile=32):
    """a [M, K] @ b [K, N] as the kernels compute it: operands split into planes, one fp32 product-sum per term and K tile, added
    to an fp32 accumulator.  drop: terms (plane of a, plane of b) left out; drop_rows: K indices left out (a tap, a K tile)."""
    a, b = a.float(), b.float()
    if drop_rows is not None:
        keep = torch.ones(a.shape[1], dtype=torch.bool)
        keep[drop_rows] = False
        a, b = a[:, keep], b[keep]
    if n_planes == 3:
        ap, bp, terms = split3(a), split3(b), [t for t in TERMS if t not in drop]
    else:
        assert torch.equal(a.half().float(), a) and torch.equal(b.half().float(), b)
        ap, bp, terms = (a,), (b,), [(0, 0)]
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], ktile):
        for ta, tb in terms:
            acc = acc + ap[ta][:, k0:k0 + ktile] @ bp[tb][k0:k0 + ktile]
    return acc


# ------------------------------------------------------------------------------------------------ values
def _sign(shape, g):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


def three_plane(shape, g):
    h = 1 + 0.25 * torch.randint(0, 4, shape, generator=g).double()
    return _sign(shape, g) * (h + _sign(shape, g) * 2.0 ** -9 + _sign(shape, g) * 2.0 ** -18)


def two_plane(shape, g):
    h = 1 + 0.25 * torch.randint(0, 2, shape, generator=g).double()
    return _sign(shape, g) * (h + _sign(shape, g) * 2.0 ** -9)


def eleven_bit(shape, g):
    return _sign(shape, g) * (1 + torch.randint(0, 1024, shape, generator=g).double() * 2.0 ** -10)


def ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def nonzero_planes(x):
    """Number of non-zero bf16 planes of every element (CPU emulation of the split)."""
    return sum((p != 0).long() for p in split3(x))


def kinds(regime):
    """(generator of a, generator of b, planes of a, planes of b) of a regime."""
    pm1 = lambda s, g: _sign(s, g)                                          # noqa: E731
    return {'A3': (three_plane, pm1, 3, 1), 'B3': (pm1, three_plane, 1, 3), 'two': (two_plane, two_plane, 2, 2),
            'dense': (lambda s, g: ints(s, g, -2, 2), lambda s, g: ints(s, g, -1, 1), None, None),
            'f16': (eleven_bit, pm1, None, None)}[regime]


def operands(regime, shape_a, shape_b, g, mask_a=None, mask_b=None):
    """The two operands (fp64 tensors holding fp32 numbers) of a regime; the masks (0 / 1 tensors or None) make one of them
    sparse — the 'dense' regime ignores them.  Asserts the plane counts the regime promises."""
    ka, kb, pa, pb = kinds(regime)
    a, b = ka(shape_a, g), kb(shape_b, g)
    if pa is not None:
        assert torch.all(nonzero_planes(a) == pa) and torch.all(nonzero_planes(b) == pb)
    if regime != 'dense':
        if mask_a is not None:
            a = a * mask_a
        if mask_b is not None:
            b = b * mask_b
    assert torch.equal(a.float().double(), a) and torch.equal(b.float().double(), b)
    return a, b


def bias_for(regime, n, g):
    """A small multiple of the granule per output channel."""
    return ints((n,), g, -3, 3) * GRANULE[regime]


def assert_condition(ref, mag, regime):
    """ref: the fp64 reference; mag: sum_k |a_k b_k| + |bias| of every output (computed like ref from the absolute values)."""
    gr = GRANULE[regime]
    assert float(mag.max()) <= HEADROOM * gr, (float(mag.max()), HEADROOM * gr)
    assert torch.equal(ref, ref.float().double())
    assert torch.equal(ref / gr, torch.round(ref / gr))
    assert (ref != 0).any()


# ------------------------------------------------------------------------------------------------ sparsity patterns
def column_pattern(rows, cols, nnz, g):
    """0 / 1 mask [rows, cols] with at most nnz ones per column, among them the first and the last row."""
    m = torch.zeros(rows, cols, dtype=torch.float64)
    idx = torch.randint(0, rows, (nnz, cols), generator=g)
    idx[0], idx[1] = 0, rows - 1
    m.scatter_(0, idx, 1.0)
    return m


def site_pattern(B, H, W, C, sy, sx, nch, g):
    """0 / 1 mask [B, H, W, C]: ones only at the sites of a lattice with spacings (sy, sx) that holds the last row and the last
    column, at most nch channels per site (all of them with nch = 0) — channel C - 1 at every other lattice site, channel 0 at
    the others."""
    m = torch.zeros(B, H, W, C, dtype=torch.float64)
    ys, xs = list(range(H - 1, -1, -sy)), list(range(W - 1, -1, -sx))
    if nch == 0:
        sub = torch.ones(B, len(ys), len(xs), C, dtype=torch.float64)
    else:
        idx = torch.randint(0, C, (B, len(ys), len(xs), nch), generator=g)
        idx[..., 0] = torch.where(torch.arange(len(xs)) % 2 == 0, C - 1, 0)
        sub = torch.zeros(B, len(ys), len(xs), C, dtype=torch.float64).scatter_(3, idx, 1.0)
    m[:, ys[0] % sy::sy, xs[0] % sx::sx] = sub.flip(1, 2)
    return m


def nnz_for(regime):
    """Non-zero products per output that keep the regime inside the condition: 4 x (1.75 + 2^-9 + 2^-18) + 3 g < 8 in the
    three-plane regimes, 4 x (1.25 + 2^-9)^2 < 8 in the two-plane one; fp16: 512 x 2 + 3 g < 2048."""
    return 512 if regime == 'f16' else 4


# ------------------------------------------------------------------------------------------------ conv problems
def _odd(k):
    return k if k % 2 else k + 1


def _conv_ref(x, w, b, stride, deconv):
    from oracle import model_ref as M
    xn = x.permute(0, 3, 1, 2)
    y = M.conv2d_transpose(xn, w, b, act=False) if deconv else M.conv2d(xn, w, b, stride, act=False)
    return y.permute(0, 2, 3, 1)


def conv_forward_problem(regime, B, H, W, Cin, Cout, k, stride, deconv=False):
    """x [B,H,W,Cin], w (HWIO, conv_transpose: [4,4,Cout,Cin]), bias, the fp64 result without activation.  Sparse side:
    'B3': x, on a site lattice whose spacing is the receptive field (one site per output) with 4 channels per site; else w, 4 taps x channels
    per output channel, among them (first tap, channel 0) and (last tap, Cin - 1)."""
    g = gen('fwd', regime, B, H, W, Cin, Cout, k, stride, deconv)
    n = nnz_for(regime)
    ma = mb = None
    if regime == 'B3':
        sp = _odd(2 if deconv else k)          # the receptive field of one output, in sites of x
        ma = site_pattern(B, H, W, Cin, sp, sp, n, g)
    elif deconv:       # [4,4,Cout,Cin]: per output channel over (tap, Cin); only 4 of the 16 taps reach one output pixel
        mb = column_pattern(16 * Cin, Cout, n, g).reshape(4, 4, Cin, Cout).permute(0, 1, 3, 2)
    else:
        mb = column_pattern(k * k * Cin, Cout, n, g).reshape(k, k, Cin, Cout)
    wshape = (4, 4, Cout, Cin) if deconv else (k, k, Cin, Cout)
    x, w = operands(regime, (B, H, W, Cin), wshape, g, ma, mb)
    b = bias_for(regime, Cout, g)
    ref = _conv_ref(x, w, b, stride, deconv)
    mag = _conv_ref(x.abs().float(), w.abs().float(), b.abs().float(), stride, deconv)
    assert_condition(ref, mag, regime)
    return x, w, b, ref


def conv_dgrad_problem(regime, B, H, W, Cin, Cout, k, stride, deconv=False):
    """dz [B,Ho,Wo,Cout], w, the fp64 data gradient [B,H,W,Cin].  Sparse side: 'B3': dz, on a site lattice; else w, 4 taps x
    output channels per INPUT channel, among them (first tap, channel 0) and (last tap, Cout - 1)."""
    g = gen('dgrad', regime, B, H, W, Cin, Cout, k, stride, deconv)
    n = nnz_for(regime)
    Ho, Wo = (2 * H, 2 * W) if deconv else (-(-H // stride), -(-W // stride))
    ma = mb = None
    if regime == 'B3':
        sp = _odd(4 if deconv else -(-k // stride))      # the sites of dz that reach one input pixel
        ma = site_pattern(B, Ho, Wo, Cout, sp, sp, n, g)
    elif deconv:
        mb = column_pattern(16 * Cout, Cin, n, g).reshape(4, 4, Cout, Cin)
    else:
        mb = column_pattern(k * k * Cout, Cin, n, g).reshape(k, k, Cout, Cin).permute(0, 1, 3, 2)
    wshape = (4, 4, Cout, Cin) if deconv else (k, k, Cin, Cout)
    dz, w = operands(regime, (B, Ho, Wo, Cout), wshape, g, ma, mb)

    def dgrad(dz_, w_):
        x0 = torch.zeros(B, H, W, Cin, dtype=dz_.dtype, requires_grad=True)
        y = _conv_ref(x0, w_, None, stride, deconv)
        return torch.autograd.grad(y, x0, dz_)[0]
    ref = dgrad(dz, w)
    assert_condition(ref, dgrad(dz.abs().float(), w.abs().float()), regime)
    return dz, w, ref


def conv_wgrad_problem(regime, B, H, W, Cin, Cout, k, stride, deconv=False):
    """x [B,H,W,Cin] (conv_transpose: the half-size input), dz, the fp64 filter gradient.  The sparse operand is dz: 4 non-zero
    sites per output channel over the whole batch, among them the first and the last site; 'dense' keeps every site."""
    g = gen('wgrad', regime, B, H, W, Cin, Cout, k, stride, deconv)
    Ho, Wo = (2 * H, 2 * W) if deconv else (-(-H // stride), -(-W // stride))
    mb = column_pattern(B * Ho * Wo, Cout, nnz_for(regime), g).reshape(B, Ho, Wo, Cout)
    x, dz = operands(regime, (B, H, W, Cin), (B, Ho, Wo, Cout), g, None, mb)
    ref = wgrad_ref(x, dz, k, stride, deconv)
    assert_condition(ref, wgrad_ref(x.abs().float(), dz.abs().float(), k, stride, deconv), regime)
    return x, dz, ref


def wgrad_ref(x, dz, k, stride, deconv=False):
    """Filter gradient as one GEMM per tap (the dtype of the inputs): conv (TF SAME) dw[ky,kx,ci,co] = sum_sites xpad[s y + ky, s x + kx, ci]
    dz[y, x, co]; conv_transpose (k 4, stride 2, y[2 i + ky - 1, 2 j + kx - 1] += x[i, j] w[ky, kx]) dw[ky,kx,co,ci]."""
    from oracle import model_ref as M
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dz.shape
    if deconv:
        big, small, s, (n0, n1) = F.pad(dz, (0, 0, 1, 1, 1, 1)), x, 2, (H, W)
    else:
        pt, pb = M.same_pads(H, k, stride)
        pl, pr = M.same_pads(W, k, stride)
        big, small, s, (n0, n1) = F.pad(x, (0, 0, pl, pr + stride, pt, pb + stride)), dz, stride, (Ho, Wo)
    sm = small.reshape(-1, small.shape[-1])
    taps = [big[:, ky:ky + s * n0:s, kx:kx + s * n1:s].reshape(-1, big.shape[-1]).t() @ sm for ky in range(k) for kx in range(k)]
    return torch.stack(taps).reshape(k, k, big.shape[-1], small.shape[-1])


# ------------------------------------------------------------------------------------------------ correlation
def corr_geometry(H, W, md, pad, s2):
    r = md // s2
    return (2 * r + 1) ** 2, H + 2 * pad - 2 * md, W + 2 * pad - 2 * md, r


def corr_forward_ref(f0, f1, md, pad, s2):
    """Cost volume of kernel_size 1, stride_1 1 (NHWC, the dtype of the inputs): out[n,oy,ox,ch] = sum_c f0[n,y,x,c] f1[n,y+dy,x+dx,c]
    / C with y = oy + md - pad, (dy, dx) = ((ch // gw - r) s2, (ch % gw - r) s2), zeros outside the images."""
    N, H, W, C = f0.shape
    oc, oh, ow, r = corr_geometry(H, W, md, pad, s2)
    P0, P1 = F.pad(f0, (0, 0, pad, pad, pad, pad)), F.pad(f1, (0, 0, pad, pad, pad, pad))
    a = P0[:, md:md + oh, md:md + ow]
    out = torch.zeros(N, oh, ow, oc, dtype=f0.dtype)
    for ch in range(oc):
        dy, dx = (ch // (2 * r + 1) - r) * s2, (ch % (2 * r + 1) - r) * s2
        out[..., ch] = (a * P1[:, md + dy:md + dy + oh, md + dx:md + dx + ow]).sum(-1)
    return out / C


def corr_backward_ref(dout, f0, f1, md, pad, s2):
    """(grad0, grad1) of corr_forward_ref: the adjoint, written out."""
    N, H, W, C = f0.shape
    oc, oh, ow, r = corr_geometry(H, W, md, pad, s2)
    P0, P1 = F.pad(f0, (0, 0, pad, pad, pad, pad)), F.pad(f1, (0, 0, pad, pad, pad, pad))
    G0, G1 = torch.zeros_like(P0), torch.zeros_like(P1)
    for ch in range(oc):
        dy, dx = (ch // (2 * r + 1) - r) * s2, (ch % (2 * r + 1) - r) * s2
        d = dout[..., ch:ch + 1]
        G0[:, md:md + oh, md:md + ow] += d * P1[:, md + dy:md + dy + oh, md + dx:md + dx + ow]
        G1[:, md + dy:md + dy + oh, md + dx:md + dx + ow] += d * P0[:, md:md + oh, md:md + ow]
    return G0[:, pad:pad + H, pad:pad + W] / C, G1[:, pad:pad + H, pad:pad + W] / C


def corr_forward_problem(regime, N, C, H, W, md, pad, s2):
    """f0, f1 [N,H,W,C] (f1 already in f0's sample order) and the fp64 cost volume.  K is the channel axis: the sparse side keeps
    4 channels per site, among them channel C - 1 or channel 0.  C is a power of two: the 1 / C scale is exact."""
    assert C & (C - 1) == 0
    g = gen('corr', regime, N, C, H, W, md, pad, s2)
    m = site_pattern(N, H, W, C, 1, 1, nnz_for(regime), g)
    f0, f1 = operands(regime, (N, H, W, C), (N, H, W, C), g, m if regime == 'B3' else None, None if regime == 'B3' else m)
    ref = corr_forward_ref(f0, f1, md, pad, s2)
    assert_condition(ref * C, corr_forward_ref(f0.abs(), f1.abs(), md, pad, s2) * C, regime)
    return f0, f1, ref


def corr_backward_problem(regime, N, C, H, W, md, pad, s2):
    """dout [N,oh,ow,oc] (operand a: the band operand), one feature tensor f [N,H,W,C] (operand b) paired with itself rolled by
    N / 2 like the training step, and the fp64 gradients (g0, g1) wrt that tensor; the fused form of the kernels is g0 + g1, and the
    condition is asserted for it too.  K is the displacement axis.  Sparse side:
    'B3': dout — a lattice of output sites with one site per displacement window vertically and two horizontally, 2 channels per
    site (pad >= md: every image pixel has an output site); else the features, on such a lattice of sites (all channels: the channels do not mix)."""
    assert C & (C - 1) == 0 and pad >= md
    g = gen('corr_bwd', regime, N, C, H, W, md, pad, s2)
    oc, oh, ow, r = corr_geometry(H, W, md, pad, s2)
    ma = mb = None
    if regime == 'B3':       # per lattice site two displacement channels whose partner pixel lies inside the image
        ma = torch.zeros(N, oh, ow, oc, dtype=torch.float64)
        disp = range(-r * s2, r * s2 + 1, s2)
        for n, y, x in site_pattern(N, H, W, 1, 2 * md + 1, md + 1, 0, g)[..., 0].nonzero().tolist():
            dys, dxs = [d for d in disp if 0 <= y + d < H], [d for d in disp if 0 <= x + d < W]
            for _ in range(2):
                dy = dys[torch.randint(0, len(dys), (1,), generator=g).item()]
                dx = dxs[torch.randint(0, len(dxs), (1,), generator=g).item()]
                ma[n, y + pad - md, x + pad - md, (dy // s2 + r) * (2 * r + 1) + dx // s2 + r] = 1
    else:
        mb = site_pattern(N, H, W, C, 2 * md + 1, md + 1, 0, g)
    dout, f = operands(regime, (N, oh, ow, oc), (N, H, W, C), g, ma, mb)

    def grads(d_, f_):
        g0, g1 = corr_backward_ref(d_, f_, torch.roll(f_, -(N // 2), 0), md, pad, s2)
        return g0, torch.roll(g1, N // 2, 0)       # grad1[m] belongs to sample m = (n + N / 2) % N of the shared tensor
    g0, g1 = grads(dout, f)
    m0, m1 = grads(dout.abs(), f.abs())
    for q, m in ((g0, m0), (g1, m1), (g0 + g1, m0 + m1)):
        assert_condition(q * C, m * C, regime)
    return dout, f, (g0, g1)
