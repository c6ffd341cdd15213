"""Exact model of the fused epilogue every data gradient ends in (imports without a GPU):

    dx = (accumulate ? dx : 0) + sum;   dx[..., act_lo:act_hi] *= leaky'(activation);   planes of dx[..., pl_lo:pl_hi]

With the inputs of tests/exact_inputs.py s = base + sum is an fp32 number, the derivative is 1.0f or 0.1f, and the expected value is ONE
correctly rounded fp32 multiply: np.float32 arithmetic, compared bit for bit — there is no tolerance in this file.  The three bf16
planes of that product re-sum to it exactly (split3 asserts it), the fp16 plane is its round-to-nearest-even cast.

The derivative has two sources: an fp32 activation (slope_f32: act > 0, IEEE, denormals included) or the first 16-bit operand plane
of a tensor that has no fp32 copy (slope_bits: sign clear and magnitude bits non-zero).  How the device's bf16 / fp16 conversion
treats denormals is not assumed: the reference of the plane source is slope_bits of the plane bits READ BACK from the buffer the
kernel reads.  act_field plants the values on which the two sources can differ (SPECIALS) at listed positions.

tests/test_dgrad_epilogue_cpu.py proves on emulated wrong epilogues that the comparators below see them; tests/test_dgrad_epilogue_gpu.py
and run_dgrad of tests/test_exact_terms_gpu.py are the users."""
import numpy as np
import torch

import exact_inputs as E

SENTINEL = 0x7fc0            # bf16 quiet NaN (fp16: a NaN too): "untouched" differs from "wrote zero"
ONE, TENTH = np.float32(1.0), np.float32(0.1)


def _p(e, m=0.0):
    return np.float32(2.0 ** e * (1.0 + m))


# name, value.  No NaN.  In the torch-CPU model 2^-149 and 2^-134 are > 0 in fp32 and zero in the bf16 hi plane; 2^-25, 2^-126 and 1e-30
# are zero in fp16; every magnitude >= 2^-133 (bf16) or > 2^-25 (fp16) has the same sign test in the plane and in fp32.
SPECIALS = [("+0", np.float32(0.0)), ("-0", np.float32(-0.0)), ("+2^-149", _p(-149)), ("-2^-149", -_p(-149)), ("+2^-126", _p(-126)),
            ("-2^-126", -_p(-126)), ("2^-134", _p(-134)), ("2^-134(1+2^-10)", _p(-134, 2.0 ** -10)), ("+2^-133", _p(-133)),
            ("-2^-133", -_p(-133)), ("2^-25", _p(-25)), ("2^-25(1+2^-10)", _p(-25, 2.0 ** -10)), ("+2^-24", _p(-24)), ("-2^-24", -_p(-24)),
            ("+1e-30", np.float32(1e-30)), ("-1e-30", np.float32(-1e-30)), ("65504", np.float32(65504.0)), ("+1e5", np.float32(1e5)),
            ("-1e5", np.float32(-1e5)), ("+3e38", np.float32(3e38)), ("-3e38", np.float32(-3e38))]
BF16_AGREE = 2.0 ** -126     # from this magnitude on the plane source and the fp32 source must agree (asserted on the device)
F16_AGREE = 2.0 ** -14


def edge_channels(N, lo, hi):
    return sorted({c for c in (lo - 1, lo, hi - 1, hi) if 0 <= c < N})


def act_field(shape, lo, hi, key):
    """(act, where, special): an fp32 activation [B,H,W,N] (numpy) of normal numbers in +-[0.5, 1.5), half of them negative, with
    SPECIALS[i] planted at the pixels i and npix - 1 - i (flat pixel order: the first and the last pixel included) of every
    channel of edge_channels(N, lo, hi); where: the list of (pixel, channel, index into SPECIALS); special: bool mask of them.
    An image of fewer than 2 len(SPECIALS) pixels (the smallest flow-head cases of tests/head_cases.py) takes npix // 8 specials per
    edge channel, every edge channel another stretch of the table, and EXACTLY half of its pixels negative in every channel (a fair
    coin over 6 pixels would leave assert_conditions to luck)."""
    B, H, W, N = shape
    g = E.gen('act', key, tuple(shape), lo, hi)
    mag = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
    act = (mag * E._sign(shape, g)).float().numpy().reshape(B * H * W, N).copy()
    special = np.zeros(act.shape, dtype=bool)
    npix, K = act.shape[0], len(SPECIALS)
    if npix < 2 * K:
        K = npix // 8
        rank = torch.rand((npix, N), generator=g).argsort(0).argsort(0).numpy()
        act = (np.abs(act) * np.where(rank < (npix + 1) // 2, -1.0, 1.0)).astype(np.float32)
    where = []
    for j, c in enumerate(edge_channels(N, lo, hi)):
        for i in range(K):
            i = (j * K + i) % len(SPECIALS)
            v = SPECIALS[i][1]
            for px in (i % K, npix - 1 - i % K):
                act[px, c] = v
                special[px, c] = True
                where.append((px, c, i))
    assert not np.isnan(act).any()
    return act.reshape(shape), where, special.reshape(shape)


def slope_f32(act):
    """Derivative from the fp32 activation: act > 0 (IEEE: a positive denormal is > 0, -0 is not)."""
    return np.where(np.asarray(act, dtype=np.float32) > 0, ONE, TENTH).astype(np.float32)


def slope_bits(bits):
    """Derivative from 16-bit plane elements (bf16 hi plane or fp16) as read back from the device."""
    b = np.asarray(bits).astype(np.int64) & 0xffff
    return np.where(((b & 0x8000) == 0) & ((b & 0x7fff) != 0), ONE, TENTH).astype(np.float32)


def f32_exact(s):
    """The fp64 tensor / array s as np.float32 — asserting that nothing is lost; -0 becomes +0 (the kernels add to +0)."""
    s64 = s.double().numpy() if isinstance(s, torch.Tensor) else np.asarray(s, dtype=np.float64)
    s32 = s64.astype(np.float32) + np.float32(0.0)
    assert np.array_equal(s32.astype(np.float64), s64)
    return s32


def expected(s, slope, lo, hi):
    """np.float32: inside [lo, hi) s * slope — one correctly rounded fp32 multiply — outside it s."""
    out = f32_exact(s).copy()
    assert slope.dtype == np.float32 and out.dtype == np.float32
    if hi > lo:
        out[..., lo:hi] = out[..., lo:hi] * slope[..., lo:hi]
    return out


def expected_planes(out, P, scale=0.0):
    """Plane VALUES [P, ...] (np.float32) of the fp32 output: the exact_inputs.split3 model (P = 3; it asserts hi + mid + lo == out)
    or the fp16 round-to-nearest-even cast of scale * out (P = 1; scale 0 = 1)."""
    assert out.dtype == np.float32
    if P == 3:
        return np.stack([p.numpy() for p in E.split3(torch.from_numpy(out))])
    v = out * np.float32(scale if scale else 1.0)
    return v.astype(np.float16).astype(np.float32)[None]


def plane_values(bits, P):
    """np.float32 values of int16 plane bits (P = 3: bf16, P = 1: fp16)."""
    b = np.ascontiguousarray(np.asarray(bits)).astype(np.int16)
    if P == 3:
        return (b.astype(np.int32) << 16).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def ranges(N):
    """The [lo, hi) ranges of a tensor with N channels (N % 4 == 0): whole, the engine's aligned half, both ends inside, both ends off
    the quad grid (lo % 4 == 1, hi % 4 == 3), inside one quad, across one quad border, empty, across an 8-channel store, across the
    128-column N tile border, the last channel alone."""
    hi3 = N - (N - 3) % 4                                 # the largest hi <= N with hi % 4 == 3
    cand = [(0, N), (0, N // 2 // 4 * 4), (8, N - 8), (5, hi3), (6, 7), (3, 9), (12, 12), (60, 70), (124, 132), (N - 1, N)]
    out = []
    for lo, hi in cand:
        if 0 <= lo <= hi <= N and (lo, hi) not in out:
            out.append((lo, hi))
    assert any(lo % 4 == 1 and hi % 4 == 3 for lo, hi in out) or N < 8
    return out


def straddle_range(N):
    return [r for r in ranges(N) if r[0] % 4 == 1 and r[1] % 4 == 3][0]


def assert_conditions(act, s, lo, hi, what=""):
    """The inputs may not hide the multiply: at least 3/4 of the in-range elements have s != 0, and in each of the channels lo - 1,
    lo, hi - 1, hi at least 1/4 of the pixels have a negative activation AND s != 0."""
    s = f32_exact(s)
    N = s.shape[-1]
    nz = s != 0
    if hi > lo:
        frac = nz[..., lo:hi].mean()
        assert frac >= 0.75, "%s: only %.3f of the elements of [%d, %d) have s != 0" % (what, frac, lo, hi)
    for c in edge_channels(N, lo, hi):
        frac = ((act[..., c] < 0) & nz[..., c]).mean()
        assert frac >= 0.25, "%s: channel %d: only %.3f of the pixels have a negative activation and s != 0" % (what, c, frac)


# ------------------------------------------------------------------------------------------------------------------ comparators
def _report(bad, got, want, what):
    idx = np.argwhere(bad)
    per_axis = [len(np.unique(idx[:, d])) for d in range(idx.shape[1])]
    first = tuple(idx[0])
    raise AssertionError("%s: %d of %d elements differ; first at %s (pixel %s, channel %d): got %r, exact %r; distinct indices per axis %s "
                         "of shape %s; channels %s" % (what, int(bad.sum()), bad.size, list(first), list(first[:-1]), first[-1],
                                                       got[first], want[first], per_axis, list(bad.shape),
                                                       np.unique(idx[:, -1])[:12].tolist()))


def _differs(got, want):
    """Element-wise 'not the same number' (a NaN on either side differs; -0 == +0)."""
    return ~(got == want)


def assert_output(buf, want, N, sentinel, what):
    """buf: the WHOLE fp32 destination buffer [..., >= N] (torch or numpy); its channels [0, N) must equal `want` everywhere, the
    channels beyond N must still hold `sentinel`."""
    got = buf.detach().cpu().numpy() if isinstance(buf, torch.Tensor) else np.asarray(buf)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape[:-1] == want.shape[:-1] and want.shape[-1] == N
    bad = _differs(got[..., :N], want)
    if bad.any():
        _report(bad, got[..., :N], want, what)
    over = _differs(got[..., N:], np.float32(sentinel))
    if over.any():
        _report(over, got[..., N:], np.full(over.shape, sentinel, dtype=np.float32), what + ": sentinel beyond N")


def assert_planes(pl_bits, want_vals, pl_lo, pl_hi, what):
    """pl_bits: int16 [P, ..., Cp] — every plane buffer pre-filled with SENTINEL before the call; want_vals: expected_planes of the
    expected output [P, ..., N].  Inside [pl_lo, pl_hi) every plane must hold its value, outside it (pad channels included) the
    sentinel pattern must be untouched."""
    bits = pl_bits.detach().cpu().numpy() if isinstance(pl_bits, torch.Tensor) else np.asarray(pl_bits)
    P = bits.shape[0]
    assert want_vals.shape[0] == P
    if pl_hi > pl_lo:
        got = plane_values(bits[..., pl_lo:pl_hi], P)
        want = want_vals[..., pl_lo:pl_hi]
        bad = _differs(got, want)
        if bad.any():
            _report(bad, got, want, what + ": planes (axis 0 = plane)")
    keep = np.ones(bits.shape[-1], dtype=bool)
    keep[pl_lo:max(pl_lo, pl_hi)] = False
    outside = (bits[..., keep].astype(np.int64) & 0xffff) != SENTINEL
    if outside.any():
        _report(outside, bits[..., keep], np.full(outside.shape, SENTINEL), what + ": planes written outside [%d, %d)" % (pl_lo, pl_hi))


# ------------------------------------------------------------------------------------------------------------------ the case table
# One row per epilogue implementation, at the smallest case of the tables of tests/test_exact_terms_gpu.py / test_planes_gpu.py that
# reaches it (read off the planners: run_pl_gather / plan_pl_gather / plan_pl_halo in csrc/conv_planes.hip, pl_halo_sk_ok in
# csrc/conv_streamk.hip, unflow_conv2d_bwd_data_po / plan_gather in csrc/conv_igemm.hip; confirmed by kernel name in a kernel trace of
# tests/test_dgrad_epilogue_gpu.py, one process per row).  N = Cin is the GEMM's column count.
#   id, entry ('pl': operand planes, 'f32': inline split), library options, (B, H, W, Cin, Cout, k, stride), conv_transpose, planes
GATHER = dict(halo=0, gather_pp=0, streamk=0)
ROWS = [
    # 10 x 14 sites: no halo tile fits; N = 36: four 8-channel stores and one 4-channel store per row (epi_store8 / epi_store4)
    ("gather", 'pl', GATHER, (1, 10, 14, 36, 40, 3, 1), False, 3),
    # The ping-pong kernel runs its own final epilogue only with the 128 x 128 tile unsplit: more than 128 tile pairs.  (2, 16, 24, 64,
    # 128, 5, 2) has N = 64 (the 128 x 64 tile: never ping-pong), the other small cases split K and end in the reduce kernel; this
    # is the smallest table case with 192 pairs.
    ("gather_pp2", 'pl', dict(halo=0, gather_pp=2, streamk=0), (4, 48, 64, 476, 256, 3, 1), False, 3),
    ("halo", 'pl', dict(streamk=0), (1, 10, 40, 128, 96, 3, 1), False, 3),             # 6 blocks, 27 K tiles: unsplit, fused epilogue
    ("streamk2", 'pl', dict(streamk=2), (1, 10, 40, 128, 96, 3, 1), False, 3),
    ("streamk2_256", 'pl', dict(streamk=2), (2, 8, 32, 256, 256, 3, 1), False, 3),
    ("s2_parity_streamk0", 'pl', dict(streamk=0), (1, 38, 70, 40, 96, 3, 2), False, 3),
    ("s2_parity", 'pl', dict(), (1, 38, 70, 40, 96, 3, 2), False, 3),
    ("splitk_reduce", 'pl', dict(), (8, 6, 8, 512, 1024, 3, 2), False, 3),             # 3 x 4 sites per class: gather, 16 slices, reduce kernel
    # 6 tiles < 384: the four-class gather form (stream-K never applies to it).  It splits K and ends in the reduce kernel; with
    # gather_max_split = 1 the gather kernel runs the epilogue itself.
    ("deconv_gather_streamk0", 'pl', dict(streamk=0), (1, 9, 40, 128, 72, 4, 2), True, 3),
    ("deconv_gather_streamk2", 'pl', dict(streamk=2), (1, 9, 40, 128, 72, 4, 2), True, 3),
    ("deconv_gather_unsplit", 'pl', dict(streamk=0, gather_max_split=1), (1, 9, 40, 128, 72, 4, 2), True, 3),
    # the accumulating-class halo form is taken from 384 tiles up or with halo_s2 = 2 (pl_halo_acc_pays): this case has 96.  One-shot
    # it splits over channel chunks (halo kernel + reduce kernel); halo_max_split = 1: the halo kernel's own epilogue.
    ("deconv_halo_acc_streamk0", 'pl', dict(streamk=0, halo_s2=2), (2, 24, 64, 388, 64, 4, 2), True, 3),
    ("deconv_halo_acc_unsplit", 'pl', dict(streamk=0, halo_s2=2, halo_max_split=1), (2, 24, 64, 388, 64, 4, 2), True, 3),
    ("deconv_halo_acc_streamk2", 'pl', dict(streamk=2, halo_s2=2), (2, 24, 64, 388, 64, 4, 2), True, 3),
    ("f16_halo", 'pl', dict(f16_k64=0, halo_s2=2), (1, 16, 32, 388, 64, 3, 1), False, 1),
    ("f16_k64_2", 'pl', dict(f16_k64=2, halo_s2=2), (1, 16, 32, 388, 64, 3, 1), False, 1),
    ("f16_db1", 'pl', dict(f16_db=1, f16_k64=0, halo_s2=2), (1, 16, 32, 388, 64, 3, 1), False, 1),
    ("f16_tall2", 'pl', dict(f16_tall=2, f16_db=0, f16_k64=0, halo_s2=2), (1, 10, 40, 388, 160, 3, 1), False, 1),
    ("f16_tall2_db1", 'pl', dict(f16_tall=2, f16_db=1, f16_k64=0, halo_s2=2), (1, 10, 40, 388, 160, 3, 1), False, 1),
    # (the two rows above split over channel chunks and end in the reduce kernel; this one is the tall kernel's own epilogue)
    ("f16_tall2_unsplit", 'pl', dict(f16_tall=2, f16_db=0, f16_k64=0, halo_s2=2, halo_max_split=1), (1, 10, 40, 388, 160, 3, 1), False, 1),
    # conv_igemm.hip.  1 x 1 x 32 takes the pointwise kernel whenever every pitch is a multiple of 4; an activation of pitch N + 1
    # forces the gather kernel (6 blocks, one K tile: unsplit, the inline epilogue).
    ("inline_gather", 'f32', dict(), (2, 12, 16, 256, 32, 1, 1), False, 3),
    ("inline_reduce", 'f32', dict(), (8, 6, 8, 512, 1024, 3, 2), False, 3),            # vector reduce kernel; scalar one with pitch N + 1
    # Cout = 2 heads (tests/head_cases.py): W % 4 == 0 and fewer than 16384 pixels: strips of 4; an activation of pitch N + 1 falls
    # back to the per-pixel (skinny) kernel.
    ("head_strip", 'f32', dict(), (2, 6, 8, 1028, 2, 3, 1), False, 3),
    ("head_strip_196", 'f32', dict(), (2, 12, 16, 196, 2, 3, 1), False, 3),
    # 16896 pixels, W % 8 == 0: strips of 8, whose range test is quad-granular (n + 3 >= act_lo && n < act_hi, then per element)
    ("head_tile8", 'f32', dict(), (2, 66, 128, 196, 2, 3, 1), False, 3),
    # W % 4 != 0: the per-pixel kernel at every pitch
    ("head_skinny", 'f32', dict(), (1, 10, 14, 196, 2, 3, 1), False, 3),
    ("pointwise", 'f32', dict(), (2, 12, 16, 256, 32, 1, 1), False, 3),
]
FORCE_PITCH = {"inline_gather"}                     # rows whose fp32 activation always has pitch N + 1
GRAD_SCALE = 4096.0


BIG = {"gather_pp2"}                                # 5.8 M outputs: 'dense' only, the ranges that cross a store or tile border


def regimes(P, name=None):
    """'dense' plus one plane regime."""
    if name in BIG:
        return ('dense',)
    return ('dense', 'A3') if P == 3 else ('dense', 'f16')


def row_ranges(name, N):
    rs = ranges(N)
    if name in BIG:
        rs = [r for r in rs if r in ((0, N), straddle_range(N), (60, 70), (124, 132))]
    return rs


def problems():
    """Every (regime, case, conv_transpose) the GPU tests use, once."""
    out = []
    for name, entry, opts, case, deconv, P in ROWS:
        for regime in regimes(P, name):
            if (regime, case, deconv) not in out:
                out.append((regime, case, deconv))
    return out


def problem(regime, case, deconv):
    """(dz, w, ref, base): the exact data-gradient problem of tests/exact_inputs.py and the accumulate base of run_dgrad."""
    B, H, W, Cin = case[:4]
    dz, w, ref = E.conv_dgrad_problem(regime, *case, deconv=deconv)
    base = E.ints((B, H, W, Cin), E.gen('base', regime, case), -3, 3) * E.GRANULE[regime]
    return dz, w, ref, base
