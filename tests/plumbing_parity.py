"""Shapes, input builders, fp64 / fp32 references and comparators of the per-element parity tests of the kernels AROUND the
network (tests/test_plumbing_kernels_gpu.py, proven without a GPU by tests/test_plumbing_parity_cpu.py): the stage-input
kernels (unflow_stack_input / _bwd / _pair / _pair_bwd), Adam and the L2 / EPE sums, the batched bias sums, the in-place
leaky-ReLU gradient and unflow_resize_bilinear_tf1.  Not a test file.

References are the oracle's own expressions (oracle/model_ref.py) in fp64, and in fp32 as the yardstick of what fp32 arithmetic
delivers on the same inputs; every input is an fp32 tensor and the oracle gets its .double().  The comparators are
loss_parity's (max_rel, check_grad, check_loss, grad_bound); the Adam parameter update adds the one quantity they do not
have (check_update).  The `standin_*` functions are fp32 torch transcriptions of the same expressions with switchable faults:
the mutants the CPU proof must see rejected."""
import functools
import math

import torch

import loss_parity as L
from oracle import model_ref as M

F32, F64 = torch.float32, torch.float64
FSCALE = 4.0 * M.FLOW_SCALE            # flownet.py:48: the coarse flow, upsampled, times 4 * FLOW_SCALE

# ================================================================================================ 1. stage input
# name -> (N, H, W, h, w): the [N,H,W,4] network input and the [N,h,w,2] flow of the previous network
STAGE_SHAPES = {
    'RAGGED': (4, 19, 45, 5, 12),       # non-dyadic ratios 5/19 and 4/15
    'QUARTER': (6, 20, 44, 5, 11),      # 1/4, B = 3
    'HALF': (6, 22, 46, 11, 23),        # 1/2
    'ODD': (3, 24, 40, 6, 10),          # 1/4, odd batch: shift != N/2
    'SAME': (2, 12, 20, 12, 20),        # 1: lx = ly = 0, x1 / y1 clamp on the whole last row / column
    'TINY': (2, 2, 3, 1, 1),            # 1/2 and 1/3: a single coarse pixel
    'BIG': (2, 332, 796, 83, 199),      # 1/4; 528,544 px > 2048 * 256: every thread makes a second pass
}
# (shape, flow set of loss_parity.SETS, pair_shift).  Non-dyadic ratios go with the near sets only: with far flows the fp32
# oracle's own upsampled flow is 1e-3 px from fp64 (position rounding x 100 px / cell), which flips floor().
STAGE_CASES = [('RAGGED', 'm1.5', 2), ('RAGGED', 'm4.0', 2), ('QUARTER', 'far', 3), ('HALF', 'far', 3), ('ODD', 'm4.0', 1),
               ('SAME', 'far', 1), ('TINY', 'm1.5', 1), ('BIG', 'm1.5', 1), ('BIG', 'far', 1)]
STAGE_VARIANTS = ('directed', 'pair')
STAGE_LD = (14, 16, 20)                 # ld_out of the 14-channel form; the 6-channel form (prev == NULL) runs at 6 and 8
NONSMOOTH_MARGIN = 1e-4                 # frac(u), frac(v) this close to {0, 1}, or min_c |warp - first| below it: d_out[8:14] = 0
NONSMOOTH_SHARE_CAP = 5e-3
FWD_FLOOR = 1e-6                        # channels 6..7 and 8..13, of the group's max
BWD_FLOOR = 2e-5                        # d_prev: float atomics, ~16 contributions per coarse pixel at ratio 1/4
# a prefilled d_prev adds one operand of the gradient's own magnitude to every atomic sum: <= 64 adds per coarse pixel (7 x 7
# fine pixels reach one at ratio 1/4), each rounding at 2^-24 of at most twice the tensor's max
PREFILL_EXTRA = 64 * 2.0 ** -24 * 2


def _stage_gen(name, kind):
    s = L.SETS[kind]
    return torch.Generator().manual_seed(s['seed'] * 1000 + STAGE_SHAPES[name][1] + 77)


@functools.lru_cache(maxsize=None)
def make_stage_inputs(name, kind):
    """im [N,H,W,3] (mean-subtracted range), prev [N,h,w,2] = flow / FSCALE with the flow drawn as loss_parity._draw_flow
    does (randn * mag; 'far': a fifth of the coarse pixels at +-50 px), d_out [N,H,W,14] before the non-smooth pixels go."""
    N, H, W, h, w = STAGE_SHAPES[name]
    s = L.SETS[kind]
    g = _stage_gen(name, kind)
    im = torch.rand(N, H, W, 3, generator=g) - 0.5
    prev = L._draw_flow(g, (N, h, w), s['mag'], s['far'], 1.0) / FSCALE
    dout = torch.randn(N, H, W, 14, generator=g)
    return dict(N=N, H=H, W=W, h=h, w=w, im=im, prev=prev, dout=dout)


def stage_operands(name, kind, shift, variant):
    """(first, second, prev, raw d_out) of a case: directed — second = im[(n + shift) % N]; pair — first = im[:B],
    second = im[B:2B] as separate tensors (B = N // 2)."""
    inp = make_stage_inputs(name, kind)
    if variant == 'directed':
        return inp['im'], torch.roll(inp['im'], -shift, 0), inp['prev'], inp['dout']
    B = max(inp['N'] // 2, 1)
    return inp['im'][:B], inp['im'][B:2 * B], inp['prev'][:B], inp['dout'][:B]


def oracle_stage(first, second, prev, H, W):
    """model_ref.flownet._s, the train_all form: [first, second, flow, warp, |warp - first|]."""
    flow = M.resize_bilinear_tf1(prev, H, W) * 4 * M.FLOW_SCALE
    warp = M.image_warp(second, flow)
    return torch.cat([first, second, flow, warp, torch.abs(warp - first)], 3)


def nonsmooth_pixels(first, second, prev, H, W):
    """[n,H,W] bool, in fp64: floor() of the warp at an integer flow, or sign() of |warp - first| at 0."""
    out = oracle_stage(first.double(), second.double(), prev.double(), H, W)
    fr = out[..., 6:8] - out[..., 6:8].floor()
    near_int = (torch.minimum(fr, 1 - fr) < NONSMOOTH_MARGIN).any(3)
    return near_int | (out[..., 11:14].amin(3) < NONSMOOTH_MARGIN)


@functools.lru_cache(maxsize=None)
def stage_dout(name, kind, shift, variant):
    """The d_out BOTH the kernel and the reference receive (channels 8..13 zeroed at the non-smooth pixels), and their share."""
    first, second, prev, dout = stage_operands(name, kind, shift, variant)
    H, W = first.shape[1:3]
    ns = nonsmooth_pixels(first, second, prev, H, W)
    dout = dout.clone()
    dout[..., 8:14] = dout[..., 8:14].masked_fill(ns.unsqueeze(3), 0.0)
    return dout, ns.float().mean().item()


def run_stage(fn, first, second, prev, dout, dt):
    """out and d/d(prev) of (out * d_out).sum() for fn(first, second, prev, H, W) evaluated in dt."""
    H, W = first.shape[1:3]
    pv = prev.to(dt).clone().requires_grad_()
    out = fn(first.to(dt), second.to(dt), pv, H, W)
    (out * dout.to(dt)).sum().backward()
    return dict(out=out.detach(), d_prev=pv.grad)


@functools.lru_cache(maxsize=None)
def ref_stage(name, kind, shift, variant, dt):
    first, second, prev, _ = stage_operands(name, kind, shift, variant)
    return run_stage(oracle_stage, first, second, prev, stage_dout(name, kind, shift, variant)[0], dt)


class _AbsSignZeroIsOne(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.abs()

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.where(x >= 0, 1.0, -1.0).to(g.dtype)


def standin_stage(mutant=None):
    """The same expressions written out tap by tap (what the kernels do), with one fault switched on:
    'tap'   the first clamped x tap of the warp reads the neighbouring column,
    'x1'    x1 = x0 + 1 without the clamp: on the last coarse column it reads the next element in memory,
    'sign0' sign(0) = 1 in the gradient of |warp - first|.
    (The wrong partner, (n + shift + 1) % N, is a fault of the operands: stage_operands(.., shift + 1, ..).)"""
    def fn(first, second, prev, H, W):
        dt = prev.dtype
        n, h, w, _ = prev.shape

        def axis(i, o):
            src = torch.arange(o, dtype=dt) * (i / o)
            lo = torch.floor(src)
            return lo.long(), torch.clamp(lo + 1, max=i - 1).long(), src - lo

        ylo, yhi, yl = axis(h, H)
        xlo, xhi, xl = axis(w, W)
        flat = torch.cat([prev.reshape(n, h * w, 2), torch.zeros(n, 1, 2, dtype=dt)], 1)
        if mutant == 'x1':
            xhi = xlo + 1
        tap = lambda yy, xx: flat[:, (yy.view(-1, 1) * w + xx.view(1, -1)).reshape(-1)].reshape(n, H, W, 2)   # noqa: E731
        tl, tr, bl, br = tap(ylo, xlo), tap(ylo, xhi), tap(yhi, xlo), tap(yhi, xhi)
        xl_, yl_ = xl.view(1, 1, -1, 1), yl.view(1, -1, 1, 1)
        t, b = tl + (tr - tl) * xl_, bl + (br - bl) * xl_
        flow = (t + (b - t) * yl_) * 4 * M.FLOW_SCALE
        ff = torch.floor(flow).detach()
        bw, fl = flow - ff, ff.long()
        x0 = torch.arange(W).view(1, 1, W) + fl[..., 0]
        y0 = torch.arange(H).view(1, H, 1) + fl[..., 1]
        xa, xb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
        ya, yb = y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
        if mutant == 'tap':
            px = tuple((xa != x0).nonzero()[0].tolist())                # a clamped tap exists in every case that uses this
            xa = xa.clone()
            xa[px] = 1 if xa[px] == 0 else W - 2
        img = second.reshape(n, H * W, 3)
        base = torch.arange(n).view(n, 1, 1)
        gat = lambda yy, xx: img[base, yy * W + xx]                      # noqa: E731
        xw, yw = bw[..., 0:1], bw[..., 1:2]
        wa, wb, wc, wd = (1 - xw) * (1 - yw), (1 - xw) * yw, xw * (1 - yw), xw * yw
        warp = ((wa * gat(ya, xa) + wb * gat(yb, xa)) + wc * gat(ya, xb)) + wd * gat(yb, xb)
        diff = _AbsSignZeroIsOne.apply(warp - first) if mutant == 'sign0' else torch.abs(warp - first)
        return torch.cat([first, second, flow, warp, diff], 3)
    return fn


def check_stage_forward(got, r32, r64):
    """Channels 0..5 bit for bit; 6..7 and 8..13 per pixel inside grad_bound(floor 1e-6) of each group's max.  Returns the worst
    ratios and the fp32 oracle's own (flow, warp groups)."""
    got = got.detach().cpu()
    assert torch.equal(got[..., :6], r32['out'][..., :6]), "channels 0..5 are copies"
    res = []
    for lo, hi in ((6, 8), (8, 14)):
        bound, own = L.grad_bound(r32['out'][..., lo:hi], r64['out'][..., lo:hi], floor=FWD_FLOOR)
        res += [L.check_grad(got[..., lo:hi], r64['out'][..., lo:hi], bound), own]
    return tuple(res)


def check_stage_backward(got, r32, r64, extra=0.0):
    bound, own = L.grad_bound(r32['d_prev'], r64['d_prev'], floor=BWD_FLOOR)
    return L.check_grad(got, r64['d_prev'], bound + extra), own, bound


@functools.lru_cache(maxsize=None)
def make_kink_case():
    """sign(0), constructed: prev = 0, so warp = second exactly in every precision, and second == first on a checkerboard: there
    warp - first is exactly 0 and d|.| must contribute nothing.  d_out is kept whole (the point of the case)."""
    N, H, W, h, w = 2, 8, 12, 2, 3
    g = torch.Generator().manual_seed(4242)
    im = torch.rand(N, H, W, 3, generator=g) - 0.5
    board = ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2 == 0)
    im[1][board] = im[0][board]
    return dict(N=N, H=H, W=W, h=h, w=w, shift=1, im=im, prev=torch.zeros(N, h, w, 2), dout=torch.randn(N, H, W, 14, generator=g))


def kink_operands(variant):
    c = make_kink_case()
    if variant == 'directed':
        return c['im'], torch.roll(c['im'], -1, 0), c['prev'], c['dout']
    return c['im'][:1], c['im'][1:], c['prev'][:1], c['dout'][:1]


def ref_kink(variant, dt):
    return run_stage(oracle_stage, *kink_operands(variant), dt)


# ================================================================================================ 2. Adam, L2, EPE sums
ADAM_NS = [1, 3, 4, 5, 1023, 4099, 2 * 1024 * 1024 + 7]       # the last: past 4 * 2048 * 256, the vector loop strides, 3-element tail
ADAM_GSCALES = [1.0, 0.5, 0.125]



def _abi(x):
    """A hyperparameter as the C ABI's float argument carries it."""
    return float(torch.tensor(x, dtype=torch.float32))


# The hyperparameters are inputs like the tensors: fp32 numbers, which the fp64 reference gets as they are.  (The entry points
# take beta as a float and form 1 - beta from it, as TF's fp32 ApplyAdam does: 1 - fl32(0.999) is 1.29e-5 below 0.001, and an
# fp64 run at the DECIMAL 0.999 differs from any such kernel by up to 2e-3 of a step where V is small — DESIGN.md, parity status.)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_L2 = 1e-4, _abi(0.9), _abi(0.999), _abi(1e-8), _abi(0.0004)
ADAM_STEPS = (1, 2, 3)
# lo % 4 of every flat range FlowNetEngine.part_buckets() yields for 'C' and 'CSS' (weights first, every layer's weight count a
# multiple of 4): test_plumbing_parity_cpu.py recomputes it from the engine's layout
ADAM_LO_RESIDUES = (0,)
ADAM_LOS = (0, 12)                                              # slice starts t[lo:lo + n] with those residues
MOMENT_FLOOR = 1e-6
L2_NS = [5, 257, 2 * 1024 * 1024 + 7]
EPE_NPIX = [1, 255, 10434, 529470]


def adam_nregs(n):
    """Inside the first float4, inside the tail, everything, beyond n."""
    return sorted({0, 1, 2, 4 * (n // 4) + 1, n, n + 5})


def adam_cases(n):
    """(n_regularized, grad_scale): the whole product; at the 2M size every n_regularized and every grad_scale once."""
    regs = adam_nregs(n)
    if n <= 4099:
        return [(r, s) for r in regs for s in ADAM_GSCALES]
    return [(r, ADAM_GSCALES[i % 3]) for i, r in enumerate(regs)]


def adam_lr_t(t):
    """FlowNetEngine.adam_begin(lr, beta1, beta2) at step t."""
    return ADAM_LR * math.sqrt(1.0 - ADAM_B2 ** t) / (1.0 - ADAM_B1 ** t)


@functools.lru_cache(maxsize=None)
def make_adam_inputs(n):
    """Non-zero moments; one gradient per step; a block of exact zeros in g, M and V together (0 / (0 + eps)) past the middle."""
    g = torch.Generator().manual_seed(9000 + n % 9973)
    p = torch.randn(n, generator=g) * 1e-2
    m = torch.randn(n, generator=g) * 1e-3
    v = torch.rand(n, generator=g) * 1e-6
    gs = [torch.randn(n, generator=g) * 1e-3 for _ in ADAM_STEPS]
    if n >= 5:
        z0, z1 = n // 2, n // 2 + min(9, n // 4)
        for t in [m, v] + gs:
            t[z0:z1] = 0.0
    return dict(p=p, m=m, v=v, g=gs)


def _adam_run(n, n_reg, gscale, dt, step):
    inp = make_adam_inputs(n)
    st = {k: inp[k].to(dt).clone() for k in 'pmv'}
    nr = min(n_reg, n)
    out = []
    for i, t in enumerate(ADAM_STEPS):
        loss = 0.5 * ADAM_L2 * (st['p'][:nr] * st['p'][:nr]).sum().item()
        step(st, inp['g'][i].to(dt), nr, gscale, t)
        out.append(dict(p=st['p'].clone(), m=st['m'].clone(), v=st['v'].clone(), loss=loss))
    return out


def _oracle_adam_step(st, g, nr, gscale, t):
    G = g * gscale
    G[:nr] = G[:nr] + ADAM_L2 * st['p'][:nr]
    P, Mm, Vv = {'x': st['p']}, {'x': st['m']}, {'x': st['v']}
    M.adam_step_tf(P, {'x': G}, Mm, Vv, t, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS)
    st['p'], st['m'], st['v'] = P['x'], Mm['x'], Vv['x']


@functools.lru_cache(maxsize=16)
def ref_adam(n, n_reg, gscale, dt):
    """Three steps of M.adam_step_tf on G = grad_scale * g + l2 * p over the regularised prefix: per step p, m, v after it and
    the L2 term 0.5 * l2 * sum(p_pre^2) of the prefix."""
    return _adam_run(n, n_reg, gscale, dt, _oracle_adam_step)


def standin_adam(n, n_reg, gscale, mutant=None):
    """fp32, written out; mutants 'nreg' (n_regularized + 1), 'scale_after' (grad_scale applied after the L2 term), 'eps_in'
    (eps inside the square root), 'v_lin' (V updated with g where g^2 belongs)."""
    def step(st, g, nr, gscale, t):
        if mutant == 'nreg':
            nr = min(nr + 1, n)
        G = g.clone() if mutant == 'scale_after' else g * gscale
        G[:nr] = G[:nr] + ADAM_L2 * st['p'][:nr]
        if mutant == 'scale_after':
            G = G * gscale
        st['m'] = ADAM_B1 * st['m'] + (1 - ADAM_B1) * G
        st['v'] = ADAM_B2 * st['v'] + ((1 - ADAM_B2) * G if mutant == 'v_lin' else (1 - ADAM_B2) * G * G)
        den = torch.sqrt(st['v'] + ADAM_EPS) if mutant == 'eps_in' else torch.sqrt(st['v']) + ADAM_EPS
        st['p'] = st['p'] - adam_lr_t(t) * st['m'] / den
    return _adam_run(n, n_reg, gscale, F32, step)


def check_update(got, ref32, ref64, lr_t):
    """The parameter after a step, as an error of the UPDATE: max |P - P_ref64| / lr_t, bounded by twice the fp32 oracle's own
    value of it plus one ulp of max |P| over lr_t (P itself rounds to fp32).  Returns (worst, the oracle's, bound)."""
    got, r64 = got.detach().cpu().double(), ref64.double()
    own = ((ref32.double() - r64).abs().max() / lr_t).item()
    ulp = 2.0 ** (math.floor(math.log2(max(r64.abs().max().item(), 1e-30))) - 23)
    bound = 2.0 * own + ulp / lr_t
    worst = ((got - r64).abs().max() / lr_t).item()
    assert worst <= bound, ("update", worst, bound)        # NaN fails
    return worst, own, bound


def check_adam_step(got, r32, r64, t):
    """got: dict p, m, v after step t.  Returns (m ratio, v ratio, update error, its bound)."""
    res = []
    for k in 'mv':
        bound, _ = L.grad_bound(r32[k], r64[k], floor=MOMENT_FLOOR)
        res.append(L.check_grad(got[k], r64[k], bound))
    worst, _, bound = check_update(got['p'], r32['p'], r64['p'], adam_lr_t(t))
    return res[0], res[1], worst, bound


@functools.lru_cache(maxsize=None)
def make_l2_input(n):
    return torch.randn(n, generator=torch.Generator().manual_seed(3000 + n % 9973)) * 1e-2


def ref_l2(n, dt, scale=ADAM_L2):
    p = make_l2_input(n).to(dt)
    return (scale * 0.5 * (p * p).sum()).item()


@functools.lru_cache(maxsize=None)
def make_epe_inputs(npix):
    g = torch.Generator().manual_seed(5000 + npix % 9973)
    f1, f2 = torch.randn(1, 1, npix, 2, generator=g) * 4, torch.randn(1, 1, npix, 2, generator=g) * 4
    mask = (torch.rand(1, 1, npix, 1, generator=g) > 0.3).float() * torch.rand(1, 1, npix, 1, generator=g)
    if npix == 1:
        mask[:] = 0.625
    return f1, f2, mask


def ref_epe(npix, masked, dt):
    """Numerator and denominator of M.flow_error_avg."""
    f1, f2, mask = (t.to(dt) for t in make_epe_inputs(npix))
    if not masked:
        mask = torch.ones_like(mask)
    den = mask.sum()
    return (M.flow_error_avg(f1, f2, mask) * den).item(), den.item()


# ================================================================================================ 3. bias sums, leaky gradient: exact
# (C, ld - C, npix, base offset in floats): ld = C, C + 4, C + 2 at C % 4 == 0 (scalar path), a base one float off 16 bytes
# (scalar path); npix gives 1, 2 and 256 chunks, the last one ragged.  The first and the last take the scalar path.
COLSUM_DESCS = [
    (3, 4, 131077, 0), (2, 0, 1, 0), (64, 0, 17, 0), (66, 4, 511, 0), (68, 0, 512, 0), (196, 4, 513, 0), (1024, 0, 1025, 0),
    (64, 2, 1025, 0), (68, 4, 131077, 0), (196, 0, 1025, 1), (1024, 4, 513, 0), (2, 4, 131077, 0), (64, 4, 131077, 0),
    (66, 0, 1025, 0), (68, 2, 513, 0), (196, 0, 17, 0), (1024, 2, 512, 0), (3, 0, 1, 0), (2, 0, 513, 0), (64, 0, 1, 0),
    (196, 4, 1025, 0), (68, 0, 1, 1), (1024, 0, 1, 0), (3, 4, 1025, 0), (66, 4, 17, 0), (64, 4, 512, 0), (196, 2, 511, 0),
    (68, 4, 511, 0), (2, 4, 17, 0), (1024, 4, 17, 0), (64, 0, 511, 0), (68, 0, 131077, 1),
]
COLSUM_SINGLES = [0, 6, 8, 31]            # launched alone (n = 1) as well: scalar, vector 2 chunks, vector 256 chunks, offset base


def colsum_path(C, ld, offset):
    """'vec' when the kernel may take its 16-byte path (the base of a fresh allocation is 16-byte aligned)."""
    return 'vec' if C % 4 == 0 and ld % 4 == 0 and offset % 4 == 0 else 'scalar'


def colsum_chunks(npix):
    return min(256, max(1, npix // 512))


@functools.lru_cache(maxsize=None)
def make_colsum_input(i):
    """x [npix, ld] of integers in -8 .. 8 (every fp32 partial sum is exact: |sum| <= 8 * 131077 < 2^24), padding columns 1e30 (a
    kernel that adds one is far off), and the int64 column sums as fp32."""
    C, pad, npix, _ = COLSUM_DESCS[i]
    g = torch.Generator().manual_seed(7000 + i)
    x = torch.full((npix, C + pad), 1e30)
    xi = torch.randint(-8, 9, (npix, C), generator=g)
    x[:, :C] = xi.float()
    return x, xi.sum(0).float()


def colsum_wrong_rows(i):
    """The sums a kernel gives that drops the last row, or adds it twice (the CPU proof: torch.equal sees both)."""
    x, _ = make_colsum_input(i)
    C = COLSUM_DESCS[i][0]
    xi = x[:, :C].long()
    return xi[:-1].sum(0).float(), (xi.sum(0) + xi[-1]).float()


LEAKY_SHAPE = (7711, 68, 72, 76)          # npix, C, lddy, ldy: npix * C = 524,348, just past 2048 * 256


@functools.lru_cache(maxsize=None)
def make_leaky_inputs():
    """dy [npix, lddy], y [npix, ldy] (padding: a sentinel in dy that must survive, NaN in y that must not be read); y holds 0.0,
    -0.0 and denormals of both signs.  Expected: fp32 dy * where(y > 0, 1, 0.1)."""
    npix, C, lddy, ldy = LEAKY_SHAPE
    g = torch.Generator().manual_seed(8100)
    dy = torch.full((npix, lddy), -777.25)
    y = torch.full((npix, ldy), float('nan'))
    dy[:, :C] = torch.randn(npix, C, generator=g)
    yv = torch.randn(npix, C, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45])
    idx = torch.arange(0, yv.numel(), 97)
    yv.view(-1)[idx] = special[torch.arange(len(idx)) % 6]
    yv[-1, -6:] = special                  # and in the last pixel, which a second pass reaches
    y[:, :C] = yv
    want = dy.clone()
    want[:, :C] = dy[:, :C] * torch.where(yv > 0, torch.tensor(1.0), torch.tensor(0.1))
    return dy, y, want


# ================================================================================================ 4. resize_bilinear_tf1
# name -> ((B, H, W, C), (OH, OW), scale)
RESIZE_CASES = {
    'kitti_up': ((1, 15, 23, 2), (16, 24), 1.0),
    'kitti_down': ((1, 16, 24, 3), (15, 23), 1.0),
    'engine': ((2, 83, 199, 2), (332, 796), 20.0),
    'degenerate': ((3, 1, 1, 2), (5, 7), 1.0),
    'identity': ((2, 12, 20, 2), (12, 20), 1.0),        # bit-exact
}
RESIZE_FLOOR = 1e-6


@functools.lru_cache(maxsize=None)
def make_resize_input(name):
    shape = RESIZE_CASES[name][0]
    return torch.randn(*shape, generator=torch.Generator().manual_seed(600 + shape[1] * shape[2]))


def ref_resize(name, dt):
    _, (oh, ow), scale = RESIZE_CASES[name]
    return M.resize_bilinear_tf1(make_resize_input(name).to(dt), oh, ow) * scale


def check_resize(got, name):
    r32, r64 = ref_resize(name, F32), ref_resize(name, F64)
    bound, own = L.grad_bound(r32, r64, floor=RESIZE_FLOOR)
    worst = L.check_grad(got, r64, bound)
    if name == 'identity':
        assert torch.equal(got.detach().cpu(), make_resize_input(name)), "a same-size resize is a copy"
    return worst, own, bound
