"""-m gpu: every entry point of csrc/ops_warp.hip through the C ABI, PER PIXEL, against the fp64 mirrors of tests/warp_parity.py
(proven without a GPU by tests/test_warp_parity_cpu.py) at the shapes where the kernels change path: images narrower than a
footprint, the 9 x 9 fast branch beside the clipped one, ragged source / target tiles, more than one LDS window, the grid caps
of the scatter, fill and gather kernels, five bins per scan thread, and the constructed ten-wide footprints.

Tolerance: max(1e-6, 2 x the fp32 C oracle's own distance from the mirror) of the tensor's max; ranges, indices and the box
means bit for bit.  Outputs start as NaN (a pixel a kernel skips fails), workspaces end in a sentinel.  Every test prints its
worst ratios (parity status)."""
import ctypes

import numpy as np
import pytest
import torch

import warp_parity as P
from test_planes_gpu import lib_option  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ERR_UNSUPPORTED, ERR_WORKSPACE = -7, -9
SENTINEL = 0xA5


def _api():
    from unflow_amd import _lib
    return _lib.lib(), _lib


def _ok(status, where=""):
    from unflow_amd._lib import check
    check(status, where)


def _dev(a, dev):
    return (a if isinstance(a, torch.Tensor) else torch.tensor(a)).to(dev).contiguous()      # (torch.tensor copies: the inputs are read-only)


def _nan(shape, dev):
    return torch.full(shape, float('nan'), device=dev)


def _misaligned(a, dev, lead=1):
    """A contiguous device copy of `a` that starts `lead` floats past a 16-byte boundary and ends with its allocation; NaN
    before it."""
    a = a if isinstance(a, torch.Tensor) else torch.tensor(a)
    buf = torch.full((a.numel() + lead,), float('nan'), device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() % 16 == 4 * lead and view.is_contiguous()
    return view


class _Workspace:
    """nbytes of workspace followed by 256 sentinel bytes."""

    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device=dev)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() if self.nbytes else 0)

    def check(self):
        assert bool((self.buf[self.nbytes:] == SENTINEL).all()), "written past the workspace's stated size"


# ------------------------------------------------------------------------------------------------ forward_warp: values
@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("name,kind", P.FW_CASES)
def test_forward_warp_values_per_pixel(name, kind, det, dev):
    lib, L = _api()
    inp, r = P.fw_inputs(name, kind), P.fw_ref(name, kind)
    B, H, W = inp['B'], inp['H'], inp['W']
    npx = B * H * W
    flow = _dev(inp['flow'], dev)
    bound, own = P.bound_of(r['o_out'], r['out'])
    full = lib.unflow_forward_warp_workspace_bytes(B, H, W, det)
    minimum = 8 * npx if det else 0
    assert full > minimum + 4 * npx
    outs, worst = {}, {}
    for path, nbytes in (("binned", full), ("atomics", minimum)):
        ws = _Workspace(nbytes, dev)
        for rep in range(2):
            out = _nan((B, H, W), dev)
            _ok(lib.unflow_forward_warp_fwd(L.ptr(flow), L.ptr(out), B, H, W, det, ws.ptr(), L.csz(nbytes), L.stream()), path)
            try:
                e = P.check(out, r['out'], bound)
            except AssertionError:
                print("%s/%s det=%d %s: worst pixel %s kernel %.9g mirror %.9g" % ((name, kind, det, path) + P.worst_pixel(out, r['out'])))
                raise
            worst[path] = max(worst.get(path, 0.0), e)
            if det:
                assert torch.equal(out, outs.setdefault(path, out)), (path, "not bit-reproducible")
        ws.check()
    if det:
        assert torch.equal(outs["binned"], outs["atomics"])      # the same fixed-point terms, integer sums
    print("forward_warp %s/%s det=%d: binned %.2e atomics %.2e (fp32 oracle %.2e, bound %.2e; far share %.2f)"
          % (name, kind, det, worst["binned"], worst["atomics"], own, bound, r['far_share']))


@pytest.mark.parametrize("name,kind", P.FW_CASES)
def test_forward_warp_ranges_bit_for_bit(name, kind, dev):
    lib, L = _api()
    inp, r = P.fw_inputs(name, kind), P.fw_ref(name, kind)
    B, H, W = inp['B'], inp['H'], inp['W']
    flow = _dev(inp['flow'], dev)
    rng = torch.full((B, H, W, 4), -77, dtype=torch.int32, device=dev)
    _ok(lib.unflow_forward_warp_ranges(L.ptr(flow), L.ptr(rng), B, H, W, L.stream()))
    got = rng.cpu().numpy()
    P.check_ranges(got, r['ranges'])
    if kind == 'built':
        for (px, py), _, want in P.TENTH_SOURCES[name]:
            assert got[0, py, px].tolist() == list(want)
            assert 9 in (want[1] - want[0], want[3] - want[2])


def test_forward_warp_status_codes(dev):
    lib, L = _api()
    B, H, W = P.FW_SHAPES['RAGGED']
    npx = B * H * W
    flow, out = torch.zeros(B, H, W, 2, device=dev), torch.zeros(B, H, W, device=dev)
    ws = _Workspace(8 * npx, dev)
    args = (L.ptr(flow), L.ptr(out), B, H, W, 1, ws.ptr())
    assert lib.unflow_forward_warp_fwd(*args, L.csz(8 * npx - 1), L.stream()) == ERR_WORKSPACE
    assert lib.unflow_forward_warp_fwd(*args, L.csz(8 * npx), L.stream()) == 0
    ws.check()
    # B * H * W = 2^31: refused before any launch (small dummy buffers)
    assert 65536 * 256 * 128 == 2 ** 31
    for det in (1, 0):
        assert lib.unflow_forward_warp_workspace_bytes(65536, 256, 128, det) == 0
        assert lib.unflow_forward_warp_fwd(L.ptr(flow), L.ptr(out), 65536, 256, 128, det, ws.ptr(), L.csz(8 * npx),
                                           L.stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(out.sum()) > 0 and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ forward_warp: gradient
def _fw_bwd(lib, L, dout, flow, B, H, W, dev):
    d_flow = _nan((B, H, W, 2), dev)
    _ok(lib.unflow_forward_warp_bwd(L.ptr(dout), L.ptr(flow), L.ptr(d_flow), B, H, W, L.stream()), "forward_warp_bwd")
    return d_flow


FW_BWD_CASES = [(n, k, 1) for n, k in P.FW_CASES] + [(n, k, 0) for n, k in P.FW_BWD_FORMS_CASES]


@pytest.mark.parametrize("name,kind,rows", FW_BWD_CASES)
def test_forward_warp_gradient_per_pixel(name, kind, rows, dev, lib_option):
    """rows = 1: the kernel that fetches a footprint row as 16 + 16 + 4 bytes (the default below 2 GiB); rows = 0: the dword
    kernel (library option fw_bwd_rows).  dout starts one float past a 16-byte boundary and ends with its allocation."""
    lib, L = _api()
    lib_option("fw_bwd_rows", rows)
    inp, r = P.fw_inputs(name, kind), P.fw_ref(name, kind)
    B, H, W = inp['B'], inp['H'], inp['W']
    flow, dout = _dev(inp['flow'], dev), _misaligned(inp['dout'], dev)
    bound, own = P.bound_of(r['o_d_flow'], r['d_flow'])
    d_flow = _fw_bwd(lib, L, dout, flow, B, H, W, dev)
    P.check_rejected_zero(d_flow, r['ok'])
    try:
        e = P.check(d_flow, r['d_flow'], bound)
    except AssertionError:
        print("%s/%s rows=%d: worst element %s kernel %.9g mirror %.9g" % ((name, kind, rows) + P.worst_pixel(d_flow, r['d_flow'])))
        raise
    print("forward_warp d_flow %s/%s rows=%d: %.2e (fp32 oracle %.2e, bound %.2e)" % (name, kind, rows, e, own, bound))


@pytest.mark.parametrize("rows", [1, 0])
def test_forward_warp_gradient_drops_what_the_wide_loads_bring_in(rows, dev, lib_option):
    """Footprints clipped at the right border with NaN in the columns that follow in memory, rows past y_hi, and a row load that
    runs past the tensor's end: finite and within the bound."""
    lib, L = _api()
    lib_option("fw_bwd_rows", rows)
    c = P.fw_border_case()
    B, H, W = c['B'], c['H'], c['W']
    bound, own = P.bound_of(c['o_d_flow'], c['d_flow'])
    d_flow = _fw_bwd(lib, L, _misaligned(c['dout'], dev), _dev(c['flow'], dev), B, H, W, dev)
    assert bool(torch.isfinite(d_flow).all())
    P.check_rejected_zero(d_flow, c['ok'])
    e = P.check(d_flow, c['d_flow'], bound)
    print("forward_warp d_flow border case rows=%d: %.2e (fp32 oracle %.2e, bound %.2e)" % (rows, e, own, bound))


# ------------------------------------------------------------------------------------------------ backward_warp
@pytest.mark.parametrize("shape,kind,C", P.BW_CASES)
def test_backward_warp_per_pixel(shape, kind, C, dev):
    """C = 2 (its own specialisation) and C = 5 (the generic template)."""
    lib, L = _api()
    inp, r = P.bw_inputs(shape, kind, C), P.bw_ref(shape, kind, C)
    B, H, W = inp['B'], inp['H'], inp['W']
    im, flow, dout = _dev(inp['im'], dev), _dev(inp['flow'], dev), _dev(inp['dout'], dev)
    out = _nan((B, H, W, C), dev)
    _ok(lib.unflow_backward_warp_fwd(L.ptr(im), L.ptr(flow), L.ptr(out), B, H, W, C, L.stream()))
    bound, own = P.bound_of(r['o_out'], r['out'])
    e = P.check(out, r['out'], bound)
    xy0 = torch.full((B, H, W, 2), -77, dtype=torch.int32, device=dev)
    _ok(lib.unflow_backward_warp_indices(L.ptr(flow), L.ptr(xy0), B, H, W, L.stream()))
    P.check_ranges(xy0.cpu().numpy(), r['xy0'])
    msg = "backward_warp %s/%s C=%d: out %.2e (fp32 oracle %.2e, bound %.2e)" % (shape, kind, C, e, own, bound)
    if kind != 'tiny':
        d_flow = _nan((B, H, W, 2), dev)
        _ok(lib.unflow_backward_warp_bwd(L.ptr(dout), L.ptr(im), L.ptr(flow), L.ptr(d_flow), B, H, W, C, L.stream()))
        gb, gown = P.bound_of(r['o_d_flow'], r['d_flow'], inp['exclude'])
        ge = P.check(d_flow, r['d_flow'], gb, inp['exclude'])
        assert not bool(torch.isnan(d_flow).any())
        msg += "  d_flow %.2e (fp32 oracle %.2e, bound %.2e, excluded %d px)" % (ge, gown, gb, int(inp['exclude'].sum()))
    print(msg)


# ------------------------------------------------------------------------------------------------ image_warp
@pytest.mark.parametrize("kind,C,shift", P.IW_CASES)
def test_image_warp_per_pixel(kind, C, shift, dev):
    """C = 1 (its own specialisation) and C = 5 (the generic template); ld_im = C and C + 3 with NaN in the unread channels;
    pair_shift 0 / 1; accumulate_d_flow 0 / 1; d_im NULL and given."""
    lib, L = _api()
    inp = P.iw_inputs(kind, C)
    r32, r64 = P.iw_ref(kind, C, shift, F32), P.iw_ref(kind, C, shift, F64)
    B, H, W, fs = inp['B'], inp['H'], inp['W'], inp['fs']
    flow, dout = _dev(inp['flow'], dev), _dev(inp['dout'], dev)
    idx_ref = P.iw_indices(kind, C, shift)
    ex = inp['exclude']
    b_out, o_out = P.bound_of(r32['out'], r64['out'])
    worst = {}
    for ld in (C, C + 3):
        im = _nan((B, H, W, ld), dev)
        im[..., :C] = inp['im'].to(dev)
        out = _nan((B, H, W, C), dev)
        idx = torch.full((B, H, W, 4), -77, dtype=torch.int32, device=dev)
        _ok(lib.unflow_image_warp_fwd(L.ptr(im), ld, L.ptr(flow), L.cf(fs), L.ptr(out), L.ptr(idx), shift, B, H, W, C, L.stream()))
        worst['out'] = max(worst.get('out', 0.0), P.check(out, r64['out'], b_out))
        P.check_ranges(idx.cpu().numpy(), idx_ref)
        out2 = _nan((B, H, W, C), dev)
        _ok(lib.unflow_image_warp_fwd(L.ptr(im), ld, L.ptr(flow), L.cf(fs), L.ptr(out2), None, shift, B, H, W, C, L.stream()))
        assert torch.equal(out, out2)                           # idx4 = NULL changes nothing
        if kind == 'tiny':
            continue
        b_fl, o_fl = P.bound_of(r32['d_flow'], r64['d_flow'], ex)
        b_im, o_im = P.bound_of(r32['d_im'], r64['d_im'])
        for with_d_im in (False, True):
            d_im = torch.zeros(B, H, W, ld, device=dev) if with_d_im else None
            d_flow = _nan((B, H, W, 2), dev)
            _ok(lib.unflow_image_warp_bwd(L.ptr(dout), L.ptr(im), ld, L.ptr(flow), L.cf(fs), L.ptr(d_im), L.ptr(d_flow), 0, shift,
                                          B, H, W, C, L.stream()))
            worst['d_flow'] = max(worst.get('d_flow', 0.0), P.check(d_flow, r64['d_flow'], b_fl, ex))
            if with_d_im:
                worst['d_im'] = max(worst.get('d_im', 0.0), P.check(d_im[..., :C], r64['d_im'], b_im))
                assert bool((d_im[..., C:] == 0).all())          # the padding channels are not written
            g = torch.Generator().manual_seed(5)
            buf = (torch.randn(B, H, W, 2, generator=g) * r64['d_flow'].abs().max().item()).float().to(dev)
            acc = buf.clone()
            _ok(lib.unflow_image_warp_bwd(L.ptr(dout), L.ptr(im), ld, L.ptr(flow), L.cf(fs), None, L.ptr(acc), 1, shift,
                                          B, H, W, C, L.stream()))
            # accumulate_d_flow = 1: got = buf + grad, within 2 ulp of the larger operand (a skipped or doubled pixel is off by |grad|)
            tol = 2.0 ** -22 * (buf.abs() + d_flow.abs())
            assert not bool((((acc - (buf + d_flow)).abs() > tol) | torch.isnan(acc)).any())
    if kind == 'tiny':
        print("image_warp %s C=%d shift=%d: out %.2e (fp32 oracle %.2e, bound %.2e)" % (kind, C, shift, worst['out'], o_out, b_out))
    else:
        print("image_warp %s C=%d shift=%d: out %.2e (oracle %.2e, bound %.2e)  d_flow %.2e (oracle %.2e, bound %.2e)  "
              "d_im %.2e (oracle %.2e, bound %.2e)" % (kind, C, shift, worst['out'], o_out, b_out, worst['d_flow'], o_fl, b_fl,
                                                       worst['d_im'], o_im, b_im))


# ------------------------------------------------------------------------------------------------ downsample
def _downsample(lib, L, im, scale, dev):
    B, H, W, C = im.shape
    out = _nan((B, H // scale, W // scale, C), dev)
    _ok(lib.unflow_downsample_fwd(L.ptr(im), L.ptr(out), B, H, W, C, scale, L.stream()), "downsample")
    return out


@pytest.mark.parametrize("C,scale", P.DS_GENERIC_CASES)
def test_downsample_generic_kernel_bit_for_bit(C, scale, dev, oracle_lib):
    """(C, scale) outside C = 3 with scale 2 / 4: downsample_kernel.  The C oracle adds in the same order."""
    lib, L = _api()
    im = P.ds_image(2, 3 * scale, 5 * scale, C)
    out = _downsample(lib, L, _dev(im, dev), scale, dev)
    assert np.array_equal(out.cpu().numpy(), oracle_lib.downsample(im, scale))


def test_downsample_generic_kernel_second_grid_pass(dev, oracle_lib):
    lib, L = _api()
    B, H, W, C, scale = P.DS_BIG
    im = P.ds_image(B, H, W, C)
    out = _downsample(lib, L, _dev(im, dev), scale, dev)
    assert out.numel() > 2048 * 256
    assert np.array_equal(out.cpu().numpy(), oracle_lib.downsample(im, scale))


@pytest.mark.parametrize("scale", [2, 4])
def test_downsample3_unaligned_base_and_end_of_allocation(scale, dev, oracle_lib):
    """downsample3_kernel (C = 3, scale 2 / 4: 16- and 8-byte buffer loads) with the image one float past a 16-byte boundary and
    ending with its allocation: bit-identical to the generic kernel (run per channel plane) and to the oracle."""
    lib, L = _api()
    im = P.ds_image(2, 3 * scale, 5 * scale, 3, seed=scale)
    ref = oracle_lib.downsample(im, scale)
    out = _downsample(lib, L, _misaligned(im, dev), scale, dev)
    assert np.array_equal(out.cpu().numpy(), ref)
    for c in range(3):
        plane = _dev(im[..., c:c + 1], dev)
        assert torch.equal(_downsample(lib, L, plane, scale, dev)[..., 0], out[..., c])
    aligned = _downsample(lib, L, _dev(im, dev), scale, dev)
    assert torch.equal(aligned, out)


# ------------------------------------------------------------------------------------------------ resize_area
def _resize_area(lib, L, t, oh, ow, dev):
    B, H, W, C = t.shape
    out = _nan((B, oh, ow, C), dev)
    _ok(lib.unflow_resize_area(L.ptr(t), L.ptr(out), B, H, W, C, oh, ow, L.stream()), "resize_area")
    return out


def _resize_area_case(B, size, osize, C, dev):
    lib, L = _api()
    (H, W), (oh, ow) = size, osize
    t = torch.from_numpy(P.ds_image(B, H, W, C, seed=7))
    r64, r32 = P.resize_area_ref(t, oh, ow), P.resize_area_ref(t, oh, ow, F32)
    bound, own = P.bound_of(r32, r64)
    e = P.check(_resize_area(lib, L, t.to(dev), oh, ow, dev), r64, bound)
    print("resize_area %dx%d -> %dx%d C=%d: %.2e (fp32 weights %.2e, bound %.2e)" % (H, W, oh, ow, C, e, own, bound))


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("size,osize", P.RA_SIZES)
def test_resize_area_per_pixel(size, osize, C, dev):
    """Fractional ratios, upsampling (3 -> 7: a source interval inside one pixel or across two) and 1 -> 1 against the fp64 area
    weights."""
    _resize_area_case(2, size, osize, C, dev)


def test_resize_area_second_grid_pass(dev):
    B, size, osize, C = P.RA_BIG
    _resize_area_case(B, size, osize, C, dev)
