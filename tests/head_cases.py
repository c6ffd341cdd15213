"""Case table of the 'no GEMM at all' kernels of csrc/conv_igemm.hip (imports without a GPU): the Cout <= 4 flow heads, the 2 -> 2
upsamplers, pointwise32_dgrad_kernel and flow_wgrad_batched — with a Python restatement of the dispatch that decides which kernel
form a shape reaches.

The restatement (head_strip, head_wgrad_blocks, skinny_wgrad_chunks, flow_wgrad_plan of conv_igemm.hip, stream_grid of common.h, the
pointwise condition of unflow_conv2d_bwd_data_po) is a MIRROR: every case states the form and the tails it is meant to reach
(`facts`), and check_case asserts that the mirror derives the same from the shape.  A threshold that moves in the library and is
moved here makes the table fail loudly; the evidence that the library takes the same decisions is the kernel trace of
tests/test_heads_gpu.py (profiles/heads_kernel_trace.txt).

tests/test_head_cases_cpu.py checks the table, tests/test_heads_gpu.py runs it."""
import collections

import numpy as np

HT_R = 4                       # rows of a head3_fwd_tile_kernel tile
PW_S, PW_CO = 8, 32            # pointwise32_dgrad_kernel: pixels per strip, output channels
TILE8_MIN_PIXELS = 16384       # head_strip: strips of 8 from this many pixels on
STREAM_GRID_CAP = 2048         # stream_grid: blocks of 256
SKINNY_FWD_CAP = 4096          # skinny_conv_fwd_kernel: blocks of 4 waves, one pixel per wave and pass
TINY_WGRAD_CAP = 32            # tiny_deconv_wgrad_kernel: blocks of 256 pixels


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the mirror
def head_strip(B, H, W, k, Cout):
    """Strip size of the flow-head kernels: 8 / 4, or 0 = the per-pixel (skinny) kernels."""
    if k != 3 or Cout != 2:
        return 0
    if W % 8 == 0 and B * H * W >= TILE8_MIN_PIXELS:
        return 8
    return 4 if W % 4 == 0 else 0


def head_wgrad_blocks(B, H, W, Cin, S):
    """(blocks per channel-quad group, strips per wave) of head3_wgrad_strip_kernel."""
    nstrips = B * H * (W // S)
    colblocks = cdiv(Cin // 4, 64)
    blocks = min(1024, max(1, 1024 // colblocks))
    spw = max(4 if nstrips >= 4096 else 1, cdiv(nstrips, blocks * 4))
    return cdiv(nstrips, spw * 4), spw


def skinny_wgrad_chunks(npix, Cin):
    colblocks = cdiv(Cin // 4, 64)
    c = cdiv(4096, colblocks)
    c = min(c, max(1, npix // 8))
    return min(c, 1024)


def flow_wgrad_plan(kind, B, H, W, Cin):
    """(kind of the batched kernel, strips per wave, blocks per channel-quad group) or None: the per-layer path.
    kind: 'conv' / 'deconv' as layers.flow_wgrad_batched takes them."""
    if kind == 'deconv':
        return 2, 0, min(TINY_WGRAD_CAP, cdiv(B * H * W, 256))
    S = head_strip(B, H, W, 3, 2)
    if S == 0:
        return None
    nstrips = B * H * (W // S)
    blocks = min(256, max(1, nstrips // 16))
    spw = cdiv(nstrips, blocks * 4)
    return (0 if S == 8 else 1), spw, cdiv(nstrips, spw * 4)


def stream_grid(items, block=256):
    return max(1, min(STREAM_GRID_CAP, cdiv(items, block)))


def passes(items, grid, per_block=256):
    """Grid-stride passes of the busiest thread / wave."""
    return cdiv(items, grid * per_block)


def pointwise_form(Cout, k, stride, lddx, ld_act):
    """unflow_conv2d_bwd_data_po: the pointwise kernel (the pointers are 16-byte aligned in every test: offsets are multiples of 4)."""
    return k == 1 and stride == 1 and Cout == PW_CO and lddx % 4 == 0 and (ld_act is None or ld_act % 4 == 0)


def _wave_tail(nstrips, spw, blocks):
    """(strips of the last non-empty wave, empty waves of the last block)."""
    last = nstrips - (blocks - 1) * spw * 4
    full, rest = divmod(last, spw)
    return (rest or spw), 4 - full - (1 if rest else 0)


def head_facts(B, H, W, Cin, Cout=2, k=3):
    """What the shape reaches in the Cout <= 4 entries, read off the launch code."""
    npix, quads = B * H * W, Cin // 4
    S = head_strip(B, H, W, k, Cout)
    f = dict(form={8: 'tile8', 4: 'strip4', 0: 'skinny'}[S], npix=npix, quads=quads, groups=cdiv(quads, 64),
             last_group_lanes=quads - 64 * (cdiv(quads, 64) - 1))
    if S:
        nstrips = B * H * (W // S)
        blocks, spw = head_wgrad_blocks(B, H, W, Cin, S)
        tail, empty = _wave_tail(nstrips, spw, blocks)
        f.update(strips=nstrips, spw=spw, wgrad_blocks=blocks, last_wave_strips=tail, empty_waves=empty)
        if S == 8:
            f['last_tile_rows'] = H % HT_R or HT_R
    else:
        f['fwd_passes'] = passes(npix, min(SKINNY_FWD_CAP, cdiv(npix, 4)), 4)
        f['dgrad_passes'] = passes(npix * quads, stream_grid(npix * quads))
        f['wgrad_chunks'] = skinny_wgrad_chunks(npix, Cin)
    return f


def pointwise_facts(B, H, W, Cin):
    npix, quads = B * H * W, Cin // 4
    return dict(form='pointwise' if pointwise_form(PW_CO, 1, 1, Cin + 4, Cin) else 'gather', npix=npix, tail_strip=npix % PW_S, quads=quads,
                groups=cdiv(quads, 64), last_group_lanes=quads - 64 * (cdiv(quads, 64) - 1))


def tiny_facts(B, H, W):
    npix = B * H * W
    blocks = min(TINY_WGRAD_CAP, cdiv(npix, 256))
    return dict(form='tiny', npix=npix, fwd_passes=passes(4 * npix, stream_grid(4 * npix)), dgrad_passes=passes(npix, stream_grid(npix)),
                wgrad_blocks=blocks, wgrad_passes=passes(npix, blocks))


# ------------------------------------------------------------------------------------------------ the table
Case = collections.namedtuple("Case", "id kind shape Cout k facts")
# kind 'head': (B, H, W, Cin), stride 1;  'pointwise': (B, H, W, Cin), k 1, Cout 32;  'tiny': the conv_transpose 2 -> 2, input (B, H, W)
HEADS = [
    # the two sides of the 16384-pixel threshold
    Case("tile8_edge", 'head', (1, 128, 128, 8), 2, 3, dict(form='tile8', npix=16384, last_tile_rows=4)),
    Case("strip4_edge", 'head', (1, 127, 128, 8), 2, 3, dict(form='strip4', npix=16256)),
    # S = 8, last row tile 2 of 4 rows, 49 quads (one partial group)
    Case("tile8_ragged", 'head', (2, 66, 128, 196), 2, 3, dict(form='tile8', last_tile_rows=2, quads=49, groups=1, spw=1)),
    # S = 8, 4128 strips: spw = 4 (4128 = 258 x 16: every wave of the stand-alone kernel is full; in flow_wgrad_batched the same
    # shape has spw = 5 and a short last wave), last row tile 1 of 4, 65 quads (64 + 1)
    Case("tile8_spw4", 'head', (1, 129, 256, 260), 2, 3,
         dict(form='tile8', strips=4128, spw=4, wgrad_blocks=258, last_wave_strips=4, empty_waves=0, last_tile_rows=1, quads=65, groups=2,
              last_group_lanes=1)),
    # S = 4 at any size because W % 8 != 0; 4150 strips: spw = 4, the last block has 6 strips (waves of 4, 2, 0, 0)
    Case("strip4_spw4", 'head', (2, 83, 100, 8), 2, 3,
         dict(form='strip4', npix=16600, strips=4150, spw=4, wgrad_blocks=260, last_wave_strips=2, empty_waves=2)),
    # one strip per row, both image borders in one window, no row above or below
    Case("strip4_one", 'head', (3, 1, 4, 8), 2, 3, dict(form='strip4', strips=3, spw=1, wgrad_blocks=1, empty_waves=1)),
    # one quad: 63 clamped inactive lanes; the forward's waves 1..3 have no group
    Case("strip4_q1", 'head', (1, 5, 12, 4), 2, 3, dict(form='strip4', quads=1, groups=1, last_group_lanes=1)),
    # 257 quads: the fifth group has one lane
    Case("strip4_1028", 'head', (2, 6, 8, 1028), 2, 3, dict(form='strip4', quads=257, groups=5, last_group_lanes=1)),
    # flow6 of a 320 x 448 input
    Case("skinny_5x7", 'head', (2, 5, 7, 1028), 2, 3, dict(form='skinny', npix=70, wgrad_chunks=8, fwd_passes=1, dgrad_passes=1)),
    # W % 4 != 0 at a mid-size level
    Case("skinny_14", 'head', (1, 10, 14, 196), 2, 3, dict(form='skinny', quads=49, wgrad_chunks=17)),
    # one column
    Case("skinny_w1", 'head', (2, 3, 1, 8), 2, 3, dict(form='skinny', npix=6, wgrad_chunks=1)),
    # 16770 pixels > 4096 x 4 waves: second pass of the forward kernel
    Case("skinny_pass2", 'head', (1, 129, 130, 8), 2, 3, dict(form='skinny', npix=16770, fwd_passes=2, wgrad_chunks=1024)),
    # 551 265 items > 2048 x 256: second pass of the data gradient
    Case("skinny_dgrad_pass2", 'head', (1, 33, 65, 1028), 2, 3, dict(form='skinny', dgrad_passes=2, fwd_passes=1)),
]
# the per-pixel templates <1>, <4> and k != 3: forward and data gradient only (the filter gradient refuses them)
TEMPLATES = [
    Case("skinny_co1", 'head', (2, 5, 8, 12), 1, 3, dict(form='skinny')),
    Case("skinny_co4", 'head', (2, 5, 8, 12), 4, 3, dict(form='skinny')),
    Case("skinny_k1", 'head', (2, 5, 8, 12), 2, 1, dict(form='skinny')),
    Case("skinny_k5", 'head', (2, 5, 8, 12), 2, 5, dict(form='skinny')),
]
POINTWISE = [
    Case("pw_tail3", 'pointwise', (1, 5, 7, 256), 32, 1, dict(form='pointwise', npix=35, tail_strip=3, groups=1, last_group_lanes=64)),
    Case("pw_65quads", 'pointwise', (2, 4, 8, 260), 32, 1, dict(form='pointwise', tail_strip=0, quads=65, groups=2, last_group_lanes=1)),
    Case("pw_q1", 'pointwise', (1, 3, 3, 4), 32, 1, dict(form='pointwise', npix=9, tail_strip=1, quads=1)),
]
TINY = [
    Case("tiny_1", 'tiny', (1, 1, 1), 2, 4, dict(form='tiny', npix=1, wgrad_blocks=1)),
    Case("tiny_5x7", 'tiny', (1, 5, 7), 2, 4, dict(form='tiny', npix=35, wgrad_blocks=1)),
    # 9230 pixels > 32 x 256: the filter-gradient blocks stride
    Case("tiny_wgrad_stride", 'tiny', (2, 65, 71), 2, 4, dict(form='tiny', npix=9230, wgrad_blocks=32, wgrad_passes=2)),
    # forward items (4 per input pixel) exceed the stream_grid cap
    Case("tiny_fwd_pass2", 'tiny', (2, 257, 260), 2, 4, dict(form='tiny', fwd_passes=2, dgrad_passes=1)),
    # data-gradient items exceed the cap
    Case("tiny_dgrad_pass2", 'tiny', (2, 520, 512), 2, 4, dict(form='tiny', dgrad_passes=2)),
]
ALL = HEADS + TEMPLATES + POINTWISE + TINY
BY_ID = {c.id: c for c in ALL}
FORMS = ('tile8', 'strip4', 'skinny', 'pointwise', 'tiny')

# flow_wgrad_batched: (case id, kind of the batched kernel, strips per wave, blocks) of one batch; a second batch with skinny_5x7 has no plan
BATCH = [("tile8_ragged", 0, 4, 132), ("strip4_1028", 1, 6, 1), ("tiny_wgrad_stride", 2, 0, 32)]
BATCH_FALLBACK = ["tile8_ragged", "skinny_5x7"]


def facts_of(c):
    if c.kind == 'head':
        return head_facts(*c.shape, Cout=c.Cout, k=c.k)
    return pointwise_facts(*c.shape) if c.kind == 'pointwise' else tiny_facts(*c.shape)


def check_case(c):
    """The mirror derives every stated fact from the shape."""
    got = facts_of(c)
    for key, want in c.facts.items():
        assert got[key] == want, "%s: %s is %r in the dispatch mirror, the table states %r" % (c.id, key, got[key], want)
    return got


def conv7(c):
    """(B, H, W, Cin, Cout, k, stride) as tests/exact_inputs.py takes it; the 2 -> 2 conv_transpose: its INPUT size, k 4, stride 2."""
    if c.kind == 'tiny':
        B, H, W = c.shape
        return (B, H, W, 2, 2, 4, 2)
    B, H, W, Cin = c.shape
    return (B, H, W, Cin, c.Cout, c.k, 1)


def batch_kind(c):
    return 'deconv' if c.kind == 'tiny' else 'conv'


# ------------------------------------------------------------------------------------------------ random data (section d)
# One case per kernel form and direction; operands randn * 10^U(-3, 3) per element.  The bound of an output element that sums n
# products (plus one for the bias or the accumulated base, plus one rounding for the slope multiply) is reference_pin.gamma(n, S) with
# S = sum |terms|: it holds for ANY fp32 evaluation order, fused or not, and nothing in it is tuned.  (For n > 10^4 the second-order
# term n^2 u^2 S passes the two units of slack; the kernels' sums there are trees of partials whose depth stays far below n, and the
# plain fp32 CPU evaluation is checked against the same bound in tests/test_head_cases_cpu.py.)
RANDOM_IDS = ["tile8_ragged", "strip4_1028", "skinny_14", "pw_65quads", "tiny_wgrad_stride"]


def wide(shape, g):
    import torch
    return torch.randn(shape, generator=g, dtype=torch.float64).float().double() * \
        (10.0 ** (torch.rand(shape, generator=g, dtype=torch.float64) * 6 - 3)).float().double()


def _f32(x):
    return x.float().double()


def random_problem(c, direction):
    """fp32-valued operands (fp64 tensors), the fp64 result v, S = sum |terms| and n per element, for 'fwd' (x, w, b), 'dgrad' (dz, w,
    base, act: the accumulating call with a derivative on [0, hi)) and 'wgrad' (x, dz)."""
    import torch
    import exact_inputs as E
    B, H, W, Cin, Cout, k, stride = case = conv7(c)
    deconv = c.kind == 'tiny'
    g = E.gen('random', c.id, direction)
    Ho, Wo = (2 * H, 2 * W) if deconv else (H, W)
    wshape = (4, 4, Cout, Cin) if deconv else (k, k, Cin, Cout)
    taps = 4 if deconv else k * k                     # taps that reach one output (conv_transpose: 4 of the 16)
    if direction == 'fwd':
        x, w, b = _f32(wide((B, H, W, Cin), g)), _f32(wide(wshape, g)), _f32(wide((Cout,), g))
        v = E._conv_ref(x, w, b, stride, deconv)
        S = E._conv_ref(x.abs(), w.abs(), b.abs(), stride, deconv)
        return dict(x=x, w=w, b=b, v=v, S=S, n=taps * Cin + 1)
    if direction == 'dgrad':
        dz, w = _f32(wide((B, Ho, Wo, Cout), g)), _f32(wide(wshape, g))
        base = _f32(wide((B, H, W, Cin), g))
        act = _f32(torch.randn((B, H, W, Cin), generator=g, dtype=torch.float64))
        hi = 0 if deconv else (Cin // 2 // 4 * 4 or 2)

        def dgrad(dz_, w_):
            x0 = torch.zeros(B, H, W, Cin, dtype=torch.float64, requires_grad=True)
            return torch.autograd.grad(E._conv_ref(x0, w_, None, stride, deconv), x0, dz_)[0]
        s, S = dgrad(dz, w), dgrad(dz.abs(), w.abs())
        slope = torch.where(act > 0, 1.0, float(np.float32(0.1)))
        slope[..., hi:] = 1.0
        n = (16 if deconv else k * k) * Cout          # every input pixel of the conv_transpose meets all 16 taps
        # overwrite: n products; accumulate: one more term; the slope multiply: one more rounding
        return dict(dz=dz, w=w, base=base, act=act, hi=hi, v0=s, S0=S, n0=n, v=(base + s) * slope, S=(base.abs() + S) * slope, n=n + 2)
    assert direction == 'wgrad'
    x, dz = _f32(wide((B, H, W, Cin), g)), _f32(wide((B, Ho, Wo, Cout), g))
    return dict(x=x, dz=dz, v=E.wgrad_ref(x, dz, k, stride, deconv), S=E.wgrad_ref(x.abs(), dz.abs(), k, stride, deconv), n=B * H * W)


def bound_ratio(got, v, S, n):
    """max |got - v| / gamma(n, S) over the elements (0 / 0 counts as 0: an element without terms must be exactly zero)."""
    import reference_pin as R
    err = (got.double() - v).abs().numpy()
    bound = R.gamma(n, S.numpy())
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max())
