"""-m gpu: the fused epilogue of the data gradients — dx = (accumulate ? dx : 0) + sum, dx[..., act_lo:act_hi] *= leaky'(activation),
planes of dx[..., pl_lo:pl_hi] — with a REAL derivative, bit for bit against tests/dgrad_epilogue.py (no tolerance anywhere).

One row of D.ROWS per epilogue implementation (the table and how each case was chosen: tests/dgrad_epilogue.py).  Three axes: the
range (D.ranges: ends off the quad grid, inside one quad, empty, across an 8-channel store and the 128-column tile border, lo > 0), the
alignment (the scalar epilogues: an fp32 activation of pitch N + 1, activation planes sliced at channel 1 and at channel 2) and the
source of the derivative (fp32 activation / first operand plane).  tests/test_dgrad_epilogue_cpu.py shows that the comparators catch
an epilogue that is wrong in any of these ways and asserts the input conditions for every case used here."""
import functools

import numpy as np
import pytest
import torch

import dgrad_epilogue as D
from test_exact_terms_gpu import _set, scaled_pt
from test_planes_gpu import lib_option, make_pt, weight_planes  # noqa: F401  (lib_option: fixture)

pytestmark = pytest.mark.gpu
F32_SENTINEL = 3.0
UNSUPPORTED = -7


@functools.lru_cache(maxsize=4)
def _problem(regime, case, deconv):
    return D.problem(regime, case, deconv)


class Layer:
    """One row's data gradient on the device: operands made once, any number of epilogues run on them."""

    def __init__(self, row, regime, dev):
        from unflow_amd.core import layers as L
        self.name, self.entry, self.opts, self.case, self.deconv, self.P = row
        self.regime, self.dev = regime, dev
        B, H, W, Cin, Cout, k, stride = self.case
        dz, w, ref, base = _problem(regime, self.case, self.deconv)
        self.ref, self.base, self.s = ref, base, base + ref
        self.shape, self.N = (B, H, W, Cin), Cin
        self.DZ = scaled_pt(dz.float(), dev, D.GRAD_SCALE, extra=8) if self.P == 1 else make_pt(dz.float(), dev, self.P, extra=8)
        if self.entry == 'pl':
            self.wd, w_dir, w_tr = weight_planes(w.float(), dev, self.P)
            self.wpl = w_tr if self.deconv else w_dir
        else:
            self.wd, self.wpl = w.float().to(dev).contiguous(), None
        self.L = L

    def dest(self, fill):
        """Destination PT: sentinel 3.0 beyond N (and, for a first writer, everywhere), planes pre-filled with the NaN pattern."""
        d = self.L.PT.alloc(self.shape[:3] + (self.N + 4,), self.dev, self.P)
        d.t.fill_(F32_SENTINEL)
        d.pl.fill_(D.SENTINEL)
        if fill:
            d.t[..., :self.N] = self.base.float().to(self.dev)
        return d

    def act_f32(self, act, pitch=0):
        """The fp32 activation on the device; pitch: extra floats per pixel row (1: the scalar epilogues)."""
        buf = torch.full(self.shape[:3] + (self.N + pitch,), 1.0, device=self.dev)
        buf[..., :self.N] = torch.from_numpy(act).to(self.dev)
        return buf[..., :self.N]

    def act_planes(self, act, offset=0):
        """The activation as a PT whose planes the LIBRARY made, living at channel `offset` of a wider buffer (1: a 2-byte aligned
        plane pointer, 2: a 4-byte aligned one — both off the 8-byte grid of the vector epilogue)."""
        L = self.L
        wide = L.PT.alloc(self.shape[:3] + (offset + self.N + (8 if offset else 0),), self.dev, self.P)
        wide.t[..., offset:offset + self.N] = torch.from_numpy(act).to(self.dev)
        L.planes_from_f32(wide.t, wide.pl)
        return L.PT(wide.t[..., offset:offset + self.N], wide.pl[..., offset:offset + self.N])

    def run(self, d, accumulate, act=None, planes=False, rng=(0, 0), pl_rng=None, planes_only=False):
        """The library call; returns its status.  'pl' rows go through ctypes (the wrappers always pass pl range = act range)."""
        from unflow_amd import _lib
        from unflow_amd._lib import ptr, stream
        L = self.L
        B, H, W, Cin, Cout, k, stride = self.case
        lo, hi = rng
        dx = d.sl(0, Cin)
        if self.entry != 'pl':
            try:
                if self.deconv:
                    L.conv2d_transpose_bwd_data(self.DZ.t, self.wd, dx.t, accumulate, act, lo, hi)
                else:
                    L.conv2d_bwd_data(self.DZ.t, self.wd, dx.t, stride, accumulate, act, lo, hi)
            except _lib.UnflowError as e:
                return e.status
            return 0
        dzp, lddz = L.nhwc(self.DZ.t)[:2]
        dxp, lddx = L.nhwc(dx.t)[:2]
        if planes_only:
            dxp = ptr(None)
        ap, lda, apl = L._act_args(act, planes)
        pl_lo, pl_hi = rng if pl_rng is None else pl_rng
        if self.deconv:
            wsp, wsn = L._ws_pl(self.dev, B, 2 * H, 2 * W, Cin, Cout, 4, 2, self.P)
            return _lib.lib().unflow_conv2d_transpose_bwd_data_pl(dzp, lddz, self.DZ.planes(), ptr(self.wd), _lib.planes_of(self.wpl), dxp, lddx,
                                                                  dx.planes(), pl_lo, pl_hi, B, H, W, Cin, Cout, int(accumulate), ap, lda, apl,
                                                                  lo, hi, wsp, wsn, stream())
        wsp, wsn = L._ws_pl(self.dev, B, H, W, Cin, Cout, k, stride, self.P)
        return _lib.lib().unflow_conv2d_bwd_data_pl(dzp, lddz, self.DZ.planes(), ptr(self.wd), _lib.planes_of(self.wpl), dxp, lddx, dx.planes(),
                                                    pl_lo, pl_hi, B, H, W, Cin, Cout, k, stride, int(accumulate), ap, lda, apl, lo, hi, wsp,
                                                    wsn, stream())

    def check(self, d, want, pl_rng, what):
        what = "%s %s %s: %s" % (self.name, self.case, self.regime, what)
        D.assert_output(d.t, want, self.N, F32_SENTINEL, what)
        if self.entry == 'pl':
            D.assert_planes(d.pl, D.expected_planes(want, self.P), pl_rng[0], pl_rng[1], what)

    def fused(self, act, rng, source='f32', accumulate=True, pitch=0, offset=0, pl_rng=None, what=""):
        """Run one fused call, compare with the model, return (destination, activation PT or tensor)."""
        lo, hi = rng
        if source == 'f32':
            A = self.act_f32(act, pitch)
            slope = D.slope_f32(act)
        else:
            A = self.act_planes(act, offset)
            slope = D.slope_bits(A.pl[0].cpu().numpy())                    # the bits the kernel reads
        d = self.dest(accumulate)
        assert self.run(d, accumulate, A, source != 'f32', rng, pl_rng) == 0
        want = D.expected(self.s if accumulate else self.ref, slope, lo, hi)
        self.check(d, want, rng if pl_rng is None else pl_rng,
                   "%s [%d, %d) source %s pitch +%d offset %d accumulate %d" % (what, lo, hi, source, pitch, offset, accumulate))
        return d


def _rows():
    return [pytest.param(row, regime, id="%s-%s" % (row[0], regime)) for row in D.ROWS for regime in D.regimes(row[5], row[0])]


def _no_timeouts():
    from unflow_amd import _lib
    return _lib.lib().unflow_debug_streamk_timeouts()


@pytest.mark.parametrize("row,regime", _rows())
def test_ranges_and_sources(row, regime, dev, lib_option):
    """Every range of D.ranges(N) with the derivative from the fp32 activation and (operand-plane entries) from its first plane; the
    two agree away from the specials."""
    _set(lib_option, row[2])
    _no_timeouts()
    lay = Layer(row, regime, dev)
    pitch = 1 if lay.name in D.FORCE_PITCH else 0
    for lo, hi in D.row_ranges(lay.name, lay.N):
        act, where, special = D.act_field(lay.shape, lo, hi, (regime, lay.case))
        d = lay.fused(act, (lo, hi), pitch=pitch)
        if lay.entry == 'pl':
            d3 = lay.fused(act, (lo, hi), source='planes')
            same = ~torch.from_numpy(special).to(dev)
            assert torch.equal(d3.t[..., :lay.N][same], d.t[..., :lay.N][same]), "plane source != fp32 source away from the specials"
    assert _no_timeouts() == 0


@pytest.mark.parametrize("row", [pytest.param(r, id=r[0]) for r in D.ROWS])
def test_alignment_plane_range_unfused_and_first_writer(row, dev, lib_option):
    """'dense', the straddling range (and the whole one):
    - the scalar epilogues (an fp32 activation of pitch N + 1; activation planes at channel 1 and 2 of a wider buffer) give the bits
      of the vector epilogue;
    - a plane range that differs from the activated range;
    - accumulate without a derivative followed by leaky_bwd_inplace on the range gives the bits of the fused call, specials included;
    - a first writer (accumulate = 0) with a derivative: the sentinel in dx does not leak."""
    _set(lib_option, row[2])
    _no_timeouts()
    lay = Layer(row, 'dense', dev)
    N, big = lay.N, lay.name in D.BIG
    st = D.straddle_range(N)
    act, _, _ = D.act_field(lay.shape, st[0], st[1], ('dense', lay.case))
    pitch = 1 if lay.name in D.FORCE_PITCH else 0
    vec = lay.fused(act, st, pitch=pitch, what="vector")
    sc = lay.fused(act, st, pitch=1, what="scalar")
    assert torch.equal(sc.t, vec.t) and torch.equal(sc.pl, vec.pl)
    lay.fused(act, st, accumulate=False, pitch=pitch, what="first writer")
    if lay.entry == 'pl':
        lay.fused(act, st, source='planes', accumulate=False, what="first writer")
        for off in (1, 2):
            lay.fused(act, st, source='planes', offset=off, what="scalar")
    if big:
        assert _no_timeouts() == 0
        return
    # fused == unfused
    for rng in ((0, N), st):
        a = D.act_field(lay.shape, rng[0], rng[1], ('dense', lay.case))[0]
        f = lay.fused(a, rng, pitch=pitch, what="fused")
        u = lay.dest(True)
        assert lay.run(u, True) == 0
        A = lay.act_f32(a)
        lay.L.leaky_bwd_inplace(u.t[..., rng[0]:rng[1]], A[..., rng[0]:rng[1]])
        assert torch.equal(u.t, f.t), "fused != accumulate + leaky_bwd_inplace on [%d, %d)" % rng
    if lay.entry == 'pl':
        whole = D.act_field(lay.shape, 0, N, ('dense', lay.case))[0]
        lay.fused(act, st, pl_rng=(0, N), what="plane range")
        lay.fused(whole, (0, N), pl_rng=(4, N - 4), what="plane range")
        lay.fused(whole, (0, N), pl_rng=(5, N - 3), what="plane range")
    assert _no_timeouts() == 0


@pytest.mark.parametrize("rowname", ["gather", "f16_halo"])
def test_sign_rule_of_the_plane_source(rowname, dev, lib_option):
    """Per special: the plane bits found on the device and the slope each source took.  (a) the plane source takes slope_bits of those
    bits; (b) from 2^-126 (bf16) / 2^-14 (fp16) on the two sources agree; (c) the fp32 source follows slope_f32 on every special.  A
    positive value that vanishes in the plane gets 0.1 from the plane source: documented behaviour, not a failure."""
    row = [r for r in D.ROWS if r[0] == rowname][0]
    _set(lib_option, row[2])
    lay = Layer(row, 'dense', dev)
    N = lay.N
    act, where, special = D.act_field(lay.shape, 0, N, ('dense', lay.case))
    A = lay.act_planes(act)
    bits = A.pl[0].cpu().numpy().reshape(-1, N).astype(np.int64) & 0xffff
    s = D.f32_exact(lay.s).reshape(-1, N)
    got = {}
    for source in ('f32', 'planes'):
        d = lay.dest(True)
        assert lay.run(d, True, A if source == 'planes' else lay.act_f32(act), source == 'planes', (0, N)) == 0
        got[source] = d.t[..., :N].cpu().numpy().reshape(-1, N)
    agree = D.BF16_AGREE if lay.P == 3 else D.F16_AGREE
    taken = {}
    for px, c, i in where:
        if s[px, c] == 0:
            continue
        one, tenth = s[px, c], s[px, c] * D.TENTH
        assert one != tenth
        t = []
        for source in ('f32', 'planes'):
            v = got[source][px, c]
            assert v == one or v == tenth, (D.SPECIALS[i][0], source, v, one, tenth)
            t.append(1.0 if v == one else 0.1)
        b = int(bits[px, c])
        assert t[1] == (1.0 if D.slope_bits(np.array([b]))[0] == D.ONE else 0.1), D.SPECIALS[i][0]           # (a)
        assert t[0] == (1.0 if D.slope_f32(D.SPECIALS[i][1]) == D.ONE else 0.1), D.SPECIALS[i][0]             # (c)
        if abs(float(D.SPECIALS[i][1])) >= agree:
            assert t[0] == t[1], D.SPECIALS[i][0]                                                     # (b)
        taken.setdefault(i, set()).add((b, t[1], t[0]))
    assert sorted(taken) == list(range(len(D.SPECIALS))), "a special has s == 0 at every planted position"
    print("\n%s plane of the activation on the device (n_planes = %d)" % ("bf16 hi" if lay.P == 3 else "fp16", lay.P))
    print("%-18s %-14s %-8s %-12s %s" % ("special", "fp32 value", "bits", "plane slope", "fp32 slope"))
    for i, (name, v) in enumerate(D.SPECIALS):
        assert len(taken[i]) == 1, (name, taken[i])                        # the same at every position
        b, tp, tf = next(iter(taken[i]))
        print("%-18s %-14.6g 0x%04x   %-12.1f %.1f" % (name, float(v), b, tp, tf))


def test_refusals(dev, lib_option):
    """Status only; each returns before any launch (read: unflow_conv2d_bwd_data_pl / unflow_conv2d_transpose_bwd_data_pl return at
    their fall-back test, unflow_conv2d_transpose_bwd_data_po at its first 2 -> 2 line, run_pl_gather before it plans a launch)."""
    from unflow_amd.core import layers as L
    st = (5, 35)
    # the plane source on a call that falls back to the fp32-operand kernels of conv_igemm.hip
    for case in ((2, 12, 16, 256, 32, 1, 1), (2, 6, 8, 1028, 2, 3, 1)):
        lay = Layer(("refusal", 'pl', {}, case, False, 3), 'dense', dev)
        act = D.act_field(lay.shape, st[0], st[1], ('dense', case))[0]
        d = lay.dest(True)
        assert lay.run(d, True, lay.act_planes(act), True, st) == UNSUPPORTED
        D.assert_output(d.t, D.f32_exact(lay.base), lay.N, F32_SENTINEL, "refused call wrote")
        assert torch.all((d.pl.int() & 0xffff) == D.SENTINEL)
        assert lay.run(d, True, lay.act_f32(act), False, st) == 0           # (the same call with the fp32 source is taken)
    # 2 -> 2 conv_transpose with a derivative
    dz, w, dx = torch.ones(2, 24, 32, 2, device=dev), torch.ones(4, 4, 2, 2, device=dev), torch.full((2, 12, 16, 2), F32_SENTINEL, device=dev)
    with pytest.raises(ValueError) as e:
        L.conv2d_transpose_bwd_data(dz, w, dx, accumulate=True, act_src=torch.ones_like(dx), act_lo=0, act_hi=2)
    assert e.value.status == UNSUPPORTED and torch.all(dx == F32_SENTINEL)
    # planes-only dx (no fp32 destination) cannot accumulate
    lay = Layer([r for r in D.ROWS if r[0] == "gather"][0], 'dense', dev)
    d = lay.dest(True)
    assert lay.run(d, True, None, False, (0, 0), pl_rng=(0, lay.N), planes_only=True) == UNSUPPORTED
    assert torch.all((d.pl.int() & 0xffff) == D.SENTINEL)
    assert lay.run(d, False, None, False, (0, 0), pl_rng=(0, lay.N), planes_only=True) == 0     # (a first writer may be planes-only)
    D.assert_planes(d.pl, D.expected_planes(D.f32_exact(lay.ref), 3), 0, lay.N, "planes-only first writer")
    D.assert_output(d.t, D.f32_exact(lay.base), lay.N, F32_SENTINEL, "planes-only call wrote fp32")
