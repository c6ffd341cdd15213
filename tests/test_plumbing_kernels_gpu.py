"""-m gpu: the kernels AROUND the network through the C ABI, per element, against fp64 evaluations of the oracle's own
expressions or against exact integer results (tests/plumbing_parity.py holds the shapes, inputs, references and comparators;
tests/test_plumbing_parity_cpu.py proves them without a GPU):

* unflow_stack_input / _bwd / _pair / _pair_bwd: non-dyadic, 1/4, 1/2 and 1:1 ratios, B = 3 and an odd batch, far flows whose
  taps clamp, ld_out 14 / 16 / 20 (and 6 / 8 without a previous flow) with the padding checked untouched, one coarse pixel, and
  BIG past the 2048-block cap.  Forward: copies bit for bit, flow and warp groups inside max(1e-6, 2 x the fp32 oracle's own
  error); backward: d_prev per coarse pixel inside max(2e-5, 2 x the fp32 oracle's), from zero and on top of a known field.
  The test owns d_out and zeroes its channels 8..13 at the pixels where floor() or sign() is not smooth (in fp64, margin
  1e-4, share capped at 5e-3 by the CPU proof); nothing is excluded from the comparison.
* unflow_adam_step / _regloss: three steps from non-zero moments, M and V per element, the parameter as an error of the update;
  every n & 3 tail, n_regularized inside a float4 / inside the tail / beyond n, grad_scale 1 / 0.5 / 0.125, sliced bases; the
  hyperparameters are the fp32 values the ABI carries, on both sides.
* unflow_l2_loss, unflow_flow_error_sums: rel 1e-5 against fp64.
* unflow_colsum_batched, unflow_leaky_bwd_inplace: exact.
* unflow_resize_bilinear_tf1 against the oracle at the ratios its users rely on.

Every test prints its worst ratios (parity status)."""
import ctypes

import pytest
import torch

import loss_parity as P
import plumbing_parity as Q

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = -5, -7, -9
SENTINEL = -777.25


def _api():
    from unflow_amd import _lib
    return _lib.lib(), _lib


def _ok(status, where=""):
    from unflow_amd._lib import check
    check(status, where)


def _im4(im3, dev):
    """[n,H,W,4] network-input layout; the fourth channel is NaN: a kernel that uses it poisons its result."""
    im = torch.full(tuple(im3.shape[:3]) + (4,), float('nan'), device=dev)
    im[..., :3] = im3.to(dev)
    return im.contiguous()


def _padded(t, ld, dev, pad_value):
    """t [.., C] as a [.., ld] device tensor with pad_value in the columns past C."""
    out = torch.full(tuple(t.shape[:-1]) + (ld,), pad_value, device=dev)
    out[..., :t.shape[-1]] = t.to(dev)
    return out


class _Stage:
    """Device operands of one stage-input case and the four entry points behind one pair of calls."""

    def __init__(self, first, second, prev, variant, shift, dev, whole_im=None):
        self.lib, self.L = _api()
        self.variant, self.shift, self.dev = variant, shift, dev
        self.n, self.H, self.W = first.shape[:3]
        self.h, self.w = prev.shape[1:3]
        self.prev = prev.to(dev).contiguous()
        if variant == 'directed':
            self.im = _im4(whole_im, dev)
        else:
            self.first, self.second = _im4(first, dev), _im4(second, dev)

    def fwd(self, out, ld, with_prev=True):
        lib, L, st = self.lib, self.L, self.L.stream()
        prev = L.ptr(self.prev if with_prev else None)
        dims = (self.n, self.H, self.W, self.h, self.w, L.cf(Q.FSCALE), st)
        if self.variant == 'directed':
            _ok(lib.unflow_stack_input(L.ptr(self.im), prev, L.ptr(out), ld, self.shift, *dims), "stack_input")
        else:
            _ok(lib.unflow_stack_input_pair(L.ptr(self.first), L.ptr(self.second), prev, L.ptr(out), ld, *dims), "stack_input_pair")

    def bwd(self, dout, ld, d_prev):
        lib, L, st = self.lib, self.L, self.L.stream()
        dims = (self.n, self.H, self.W, self.h, self.w, L.cf(Q.FSCALE), st)
        if self.variant == 'directed':
            _ok(lib.unflow_stack_input_bwd(L.ptr(dout), ld, L.ptr(self.im), L.ptr(self.prev), L.ptr(d_prev), self.shift, *dims),
                "stack_input_bwd")
        else:
            _ok(lib.unflow_stack_input_pair_bwd(L.ptr(dout), ld, L.ptr(self.first), L.ptr(self.second), L.ptr(self.prev), L.ptr(d_prev),
                                                *dims), "stack_input_pair_bwd")

    def out_buffer(self, ld, C):
        out = torch.full((self.n, self.H, self.W, ld), float('nan'), device=self.dev)       # a pixel the kernel skips stays NaN
        out[..., C:] = SENTINEL
        return out


def _stage_forward_checks(s, r32, r64, tag):
    outs = []
    for ld in Q.STAGE_LD:
        out = s.out_buffer(ld, 14)
        s.fwd(out, ld)
        assert bool((out[..., 14:] == SENTINEL).all()), ("padding written", ld)
        e_flow, o_flow, e_warp, o_warp = Q.check_stage_forward(out[..., :14], r32, r64)
        print("stage fwd %s ld %d: flow %.2e (fp32 oracle %.2e)  warp, |warp - first| %.2e (fp32 oracle %.2e)"
              % (tag, ld, e_flow, o_flow, e_warp, o_warp))
        outs.append(out[..., :14].clone())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])              # the pitch changes addresses only
    for ld in (6, 8):                                                   # a first-stage S: no previous flow, 6 channels
        out = s.out_buffer(ld, 6)
        s.fwd(out, ld, with_prev=False)
        assert bool((out[..., 6:] == SENTINEL).all()), ("padding written", ld)
        assert torch.equal(out[..., :6].cpu(), r32['out'][..., :6])


def _stage_backward_checks(s, dout, r32, r64, tag):
    grads = []
    for ld in Q.STAGE_LD:
        d_prev = torch.zeros(s.n, s.h, s.w, 2, device=s.dev)
        s.bwd(_padded(dout, ld, s.dev, float('nan')), ld, d_prev)
        e, own, bound = Q.check_stage_backward(d_prev, r32, r64)
        print("stage bwd %s ld %d: d_prev %.2e (fp32 oracle %.2e, bound %.2e)" % (tag, ld, e, own, bound))
        grads.append(d_prev)
    # on top of a known field of the gradient's own magnitude: the result is that field plus the gradient
    ref = r64['d_prev']
    field = (torch.randn(ref.shape, generator=torch.Generator().manual_seed(99)) * ref.abs().max().item()).float()
    acc = field.to(s.dev)
    s.bwd(_padded(dout, 14, s.dev, 0.0), 14, acc)
    e, _, bound = Q.check_stage_backward(acc.cpu().double() - field.double(), r32, r64, Q.PREFILL_EXTRA)
    print("stage bwd %s accumulated: d_prev %.2e (bound %.2e)" % (tag, e, bound + Q.PREFILL_EXTRA))


@pytest.mark.parametrize("variant", Q.STAGE_VARIANTS)
@pytest.mark.parametrize("name,kind,shift", Q.STAGE_CASES)
def test_stage_input_kernels_per_pixel(name, kind, shift, variant, dev):
    first, second, prev, _ = Q.stage_operands(name, kind, shift, variant)
    dout, share = Q.stage_dout(name, kind, shift, variant)
    r32, r64 = Q.ref_stage(name, kind, shift, variant, F32), Q.ref_stage(name, kind, shift, variant, F64)
    s = _Stage(first, second, prev, variant, shift, dev, whole_im=Q.make_stage_inputs(name, kind)['im'])
    tag = "%s/%s %s shift %d (zeroed share %.1e)" % (name, kind, variant, shift, share)
    _stage_forward_checks(s, r32, r64, tag)
    _stage_backward_checks(s, dout, r32, r64, tag)


@pytest.mark.parametrize("variant", Q.STAGE_VARIANTS)
def test_stage_input_sign_of_zero(variant, dev):
    """warp == first exactly on half of the pixels (plumbing_parity.make_kink_case), d_out kept whole: d|.| is 0 at 0."""
    first, second, prev, dout = Q.kink_operands(variant)
    r32, r64 = Q.ref_kink(variant, F32), Q.ref_kink(variant, F64)
    s = _Stage(first, second, prev, variant, 1, dev, whole_im=Q.make_kink_case()['im'])
    _stage_forward_checks(s, r32, r64, "kink " + variant)
    _stage_backward_checks(s, dout, r32, r64, "kink " + variant)


def test_stage_input_shape_errors(dev):
    lib, L = _api()
    z = lambda *s: torch.zeros(*s, device=dev)
    im, prev, out, st = z(2, 4, 6, 4), z(2, 2, 3, 2), z(2, 4, 6, 16), L.stream()
    fs = L.cf(Q.FSCALE)
    assert lib.unflow_stack_input(L.ptr(im), L.ptr(prev), L.ptr(out), 13, 1, 2, 4, 6, 2, 3, fs, st) == ERR_SHAPE
    assert lib.unflow_stack_input(L.ptr(im), L.ptr(None), L.ptr(out), 5, 1, 2, 4, 6, 0, 0, fs, st) == ERR_SHAPE
    assert lib.unflow_stack_input(L.ptr(im), L.ptr(None), L.ptr(out), 6, 1, 2, 4, 6, 0, 0, fs, st) == 0
    assert lib.unflow_stack_input_pair(L.ptr(im), L.ptr(im), L.ptr(prev), L.ptr(out), 13, 2, 4, 6, 2, 3, fs, st) == ERR_SHAPE
    assert lib.unflow_stack_input_bwd(L.ptr(out), 13, L.ptr(im), L.ptr(prev), L.ptr(prev), 1, 2, 4, 6, 2, 3, fs, st) == ERR_SHAPE
    assert lib.unflow_stack_input_pair_bwd(L.ptr(out), 13, L.ptr(im), L.ptr(im), L.ptr(prev), L.ptr(prev), 2, 4, 6, 2, 3, fs, st) == ERR_SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ Adam
def _slice_buffer(src, lo, dev):
    """src inside a larger allocation at [lo, lo + n), sentinels around it."""
    t = torch.full((lo + src.numel() + 8,), SENTINEL, device=dev)
    t[lo:lo + src.numel()] = src.to(dev)
    return t


@pytest.mark.parametrize("n", Q.ADAM_NS)
def test_adam_kernel_per_element(n, dev):
    lib, L = _api()
    inp = Q.make_adam_inputs(n)
    st = L.stream()
    worst = dict(m=0.0, v=0.0, upd=0.0, updbound=0.0, loss=0.0)
    for case, (n_reg, gscale) in enumerate(Q.adam_cases(n)):
        r32, r64 = Q.ref_adam(n, n_reg, gscale, F32), Q.ref_adam(n, n_reg, gscale, F64)
        # both entry points on both bases; at the 2M size one of each per case, alternating (the fp64 comparisons take seconds)
        combos = [(lo, rl) for lo in Q.ADAM_LOS for rl in (False, True)]
        if n > 4099:
            combos = [combos[0], combos[3]] if case == 0 else [combos[case % 4]]
        for lo, regloss in combos:
            buf = {k: _slice_buffer(inp[k], lo, dev) for k in 'pmv'}
            sl = lambda t: L.ptr(t[lo:lo + n])                                           # noqa: E731
            for i, t in enumerate(Q.ADAM_STEPS):
                g = _slice_buffer(inp['g'][i], lo, dev)
                args = (sl(buf['p']), sl(g), sl(buf['m']), sl(buf['v']), L.cl(n), L.cl(n_reg), L.cf(gscale), L.cf(Q.ADAM_L2),
                        L.cf(Q.adam_lr_t(t)), L.cf(Q.ADAM_B1), L.cf(Q.ADAM_B2), L.cf(Q.ADAM_EPS))
                if regloss:
                    acc = torch.zeros(1, device=dev)
                    _ok(lib.unflow_adam_step_regloss(*args, L.ptr(acc), st), "adam_step_regloss")
                    worst['loss'] = max(worst['loss'], P.check_loss(acc.item(), r64[i]['loss']))
                else:
                    _ok(lib.unflow_adam_step(*args, st), "adam_step")
                got = {k: buf[k][lo:lo + n].cpu() for k in 'pmv'}
                e_m, e_v, e_u, b_u = Q.check_adam_step(got, r32[i], r64[i], t)
                worst['m'], worst['v'] = max(worst['m'], e_m), max(worst['v'], e_v)
                if e_u >= worst['upd']:
                    worst['upd'], worst['updbound'] = e_u, b_u
            for k in 'pmv':                                                              # nothing outside the slice moved
                assert bool((buf[k][:lo] == SENTINEL).all()) and bool((buf[k][lo + n:] == SENTINEL).all()), (k, lo)
    print("adam n %d: M %.2e  V %.2e (bound %.0e or 2 x fp32 oracle)  update error / lr_t %.2e (bound %.2e)  L2 term rel %.2e"
          % (n, worst['m'], worst['v'], Q.MOMENT_FLOOR, worst['upd'], worst['updbound'], worst['loss']))


@pytest.mark.parametrize("n", Q.L2_NS)
def test_l2_loss_kernel(n, dev):
    lib, L = _api()
    p = Q.make_l2_input(n).to(dev)
    acc = torch.zeros(1, device=dev)
    _ok(lib.unflow_l2_loss(L.ptr(p), L.cl(n), L.cf(Q.ADAM_L2), L.ptr(acc), L.stream()), "l2_loss")
    e = P.check_loss(acc.item(), Q.ref_l2(n, F64))
    _ok(lib.unflow_l2_loss(L.ptr(p), L.cl(n), L.cf(Q.ADAM_L2), L.ptr(acc), L.stream()), "l2_loss")     # it accumulates
    P.check_loss(acc.item(), 2 * Q.ref_l2(n, F64))
    print("l2_loss n %d: rel %.2e" % (n, e))


@pytest.mark.parametrize("npix", Q.EPE_NPIX)
def test_flow_error_sums_kernel(npix, dev):
    lib, L = _api()
    f1, f2, mask = Q.make_epe_inputs(npix)
    a, b, m = f1.reshape(npix, 2).to(dev).contiguous(), f2.reshape(npix, 2).to(dev).contiguous(), mask.reshape(npix).to(dev).contiguous()
    for masked in (False, True):
        num, den = Q.ref_epe(npix, masked, F64)
        out2 = torch.full((2,), 123.0, device=dev)                      # the entry resets its own accumulators
        for _ in range(2):
            _ok(lib.unflow_flow_error_sums(L.ptr(a), L.ptr(b), L.ptr(m if masked else None), L.ptr(out2), L.cl(npix), L.stream()),
                "flow_error_sums")
            e_n, e_d = P.check_loss(out2[0].item(), num), P.check_loss(out2[1].item(), den)
        print("flow_error_sums npix %d masked %d: numerator %.2e  denominator %.2e" % (npix, masked, e_n, e_d))


# ------------------------------------------------------------------------------------------------ bias sums, leaky gradient
class _Colsum:
    """ctypes tables of one unflow_colsum_batched launch over the descriptors `idxs` of plumbing_parity.COLSUM_DESCS."""

    def __init__(self, idxs, dev):
        self.lib, self.L = _api()
        self.lib.unflow_colsum_batched_workspace_bytes.restype = ctypes.c_size_t
        self.n = n = len(idxs)
        self.keep, self.outs, self.want = [], [], []
        xs, lds, npx, cs, ops = [], [], [], [], []
        for i in idxs:
            C, pad, npix, off = Q.COLSUM_DESCS[i]
            x, want = Q.make_colsum_input(i)
            buf = torch.full((x.numel() + off,), 1e30, device=dev)
            buf[off:] = x.reshape(-1).to(dev)
            out = torch.full((C + 4,), float('nan'), device=dev)
            out[C:] = SENTINEL
            self.keep.append(buf)
            self.outs.append(out)
            self.want.append(want)
            assert (buf.data_ptr() % 16 == 0) and Q.colsum_path(C, C + pad, off) == ('vec' if (C % 4, pad % 4, off) == (0, 0, 0) else 'scalar')
            xs.append(buf.data_ptr() + 4 * off)
            lds.append(C + pad)
            npx.append(npix)
            cs.append(C)
            ops.append(out.data_ptr())
        self.xs, self.lds = (ctypes.c_void_p * n)(*xs), (ctypes.c_int * n)(*lds)
        self.npx, self.cs, self.ops = (ctypes.c_long * n)(*npx), (ctypes.c_int * n)(*cs), (ctypes.c_void_p * n)(*ops)
        self.nbytes = int(self.lib.unflow_colsum_batched_workspace_bytes(n, self.cs))
        self.ws = torch.empty(self.nbytes // 4 + 64, dtype=F32, device=dev)

    def launch(self, n=None, lds=None, ws_bytes=None):
        L = self.L
        return self.lib.unflow_colsum_batched(self.n if n is None else n, self.xs, self.lds if lds is None else lds, self.npx, self.cs,
                                              self.ops, L.ptr(self.ws), L.csz(self.nbytes if ws_bytes is None else ws_bytes), L.stream())

    def check(self):
        for k, (out, want) in enumerate(zip(self.outs, self.want)):
            C = want.numel()
            assert bool((out[C:] == SENTINEL).all()), ("bias sum wrote past C", k)
            assert torch.equal(out[:C].cpu(), want), ("bias sum", k, int((out[:C].cpu() != want).sum()))


def test_colsum_batched_exact(dev):
    """Integer inputs: every fp32 partial sum is exact, so the result equals the int64 column sums whatever the path, the chunking
    and the order — one dropped or doubled row is a mismatch."""
    full = _Colsum(list(range(32)), dev)
    _ok(full.launch(), "colsum_batched")
    full.check()
    for i in Q.COLSUM_SINGLES:
        one = _Colsum([i], dev)
        _ok(one.launch(), "colsum_batched")
        one.check()
    # status codes
    many = _Colsum([1, 2] * 16 + [1], dev)
    assert many.n == 33 and many.launch() == ERR_UNSUPPORTED
    small = _Colsum([2, 3], dev)
    assert small.launch(ws_bytes=small.nbytes - 4) == ERR_WORKSPACE
    bad_ld = (ctypes.c_int * 2)(Q.COLSUM_DESCS[2][0], Q.COLSUM_DESCS[3][0] - 1)
    assert small.launch(lds=bad_ld) == ERR_SHAPE
    _ok(small.launch(), "colsum_batched")
    small.check()
    torch.cuda.synchronize()
    print("colsum_batched: 32 descriptors and %d single launches exact" % len(Q.COLSUM_SINGLES))


def test_leaky_bwd_inplace_exact(dev):
    lib, L = _api()
    npix, C, lddy, ldy = Q.LEAKY_SHAPE
    dy, y, want = Q.make_leaky_inputs()
    d, yy = dy.to(dev).contiguous(), y.to(dev).contiguous()
    _ok(lib.unflow_leaky_bwd_inplace(L.ptr(d), lddy, L.ptr(yy), ldy, L.cl(npix), C, L.stream()), "leaky_bwd_inplace")
    got = d.cpu()
    assert torch.equal(got[:, C:], want[:, C:]), "padding written"
    assert torch.equal(got, want), int((got != want).sum())
    print("leaky_bwd_inplace %d x %d (lddy %d, ldy %d): exact, +-0 and denormals included" % (npix, C, lddy, ldy))


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("name", list(Q.RESIZE_CASES))
def test_resize_bilinear_tf1_vs_oracle(name, dev):
    lib, L = _api()
    (B, H, W, C), (oh, ow), scale = Q.RESIZE_CASES[name]
    x = Q.make_resize_input(name).to(dev).contiguous()
    out = torch.full((B, oh, ow, C), float('nan'), device=dev)
    _ok(lib.unflow_resize_bilinear_tf1(L.ptr(x), L.ptr(out), B, H, W, C, oh, ow, L.cf(scale), L.stream()), "resize_bilinear_tf1")
    worst, own, bound = Q.check_resize(out, name)
    print("resize_bilinear_tf1 %s %dx%d -> %dx%d: %.2e (fp32 oracle %.2e, bound %.2e)" % (name, H, W, oh, ow, worst, own, bound))
