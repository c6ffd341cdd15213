"""tests/dgrad_epilogue.py has teeth (no GPU): emulated WRONG epilogues are caught by its comparators on the cases, ranges and inputs
that tests/test_dgrad_epilogue_gpu.py runs, the inputs meet the conditions that keep the multiply visible, the specials table says
what the torch model says, and the bf16 split of the expected output is exact."""
import functools

import numpy as np
import pytest
import torch

import dgrad_epilogue as D
import exact_inputs as E

SMALL = [r for r in D.ROWS if r[0] in ("gather", "halo")]            # the mutants run on these rows' cases (every range)
F32_SENTINEL = 3.0


@functools.lru_cache(maxsize=4)
def _problem(regime, case, deconv):
    return D.problem(regime, case, deconv)


def model_bits(act, P, plane=0):
    """Plane bits of the activation in the torch-CPU model (round to nearest even at every level)."""
    a = torch.from_numpy(np.ascontiguousarray(act))
    if P == 1:
        return a.half().view(torch.int16).numpy()
    for _ in range(plane):
        a = a - a.bfloat16().float()
    return a.bfloat16().view(torch.int16).numpy()


def epilogue(base, ref, act, lo, hi, source, P, mutant=None):
    """The destination buffer [..., N + 4] a kernel leaves (sentinel beyond N), computed in np.float32 like the kernels do; mutant: the
    way in which it is wrong."""
    N = act.shape[-1]
    b32, r32 = D.f32_exact(base), D.f32_exact(ref)
    slope = D.slope_f32(act) if source == 'f32' else D.slope_bits(model_bits(act, P))
    if mutant == 'lo':
        lo = lo - 1 if lo > 0 else lo + 1
    elif mutant == 'hi':
        hi = hi + 1 if hi < N else hi - 1
    elif mutant == 'quad':                                              # a straddling quad multiplied whole
        lo, hi = (lo // 4 * 4, min(N, -(-hi // 4) * 4)) if hi > lo else (lo, hi)
    elif mutant == 'ge0':
        slope = np.where(act >= 0, D.ONE, D.TENTH).astype(np.float32)
    elif mutant == 'mid':
        slope = D.slope_bits(model_bits(act, P, 1))
    elif mutant == 'ld':                                                # an activation of pitch N + 1 read with the destination's N + 4
        flat = np.ones((act.size // N, N + 1), dtype=np.float32)
        flat[:, :N] = act.reshape(-1, N)
        idx = (np.arange(flat.shape[0])[:, None] * (N + 4) + np.arange(N)[None, :]) % flat.size
        slope = D.slope_f32(flat.reshape(-1)[idx].reshape(act.shape))
    hi = max(hi, lo)
    out = np.full(act.shape[:-1] + (N + 4,), F32_SENTINEL, dtype=np.float32)
    if mutant == 'before':                                              # the derivative applied before the accumulate
        v = r32.copy()
        v[..., lo:hi] = v[..., lo:hi] * slope[..., lo:hi]
        out[..., :N] = b32 + v
    else:
        v = b32 + r32
        v[..., lo:hi] = v[..., lo:hi] * slope[..., lo:hi]
        out[..., :N] = v
    return out


def caught(buf, want, N):
    try:
        D.assert_output(buf, want, N, F32_SENTINEL, "mutant")
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------ the table
def test_specials_table_matches_the_torch_model():
    vals = np.array([v for _, v in D.SPECIALS], dtype=np.float32)
    names = [n for n, _ in D.SPECIALS]
    assert not np.isnan(vals).any() and len(set(names)) == len(names)
    f32 = D.slope_f32(vals)
    bf, fh = D.slope_bits(model_bits(vals, 3)), D.slope_bits(model_bits(vals, 1))
    row = dict(zip(names, zip(f32, bf, fh)))
    for n in ("+2^-149", "2^-134"):                                     # > 0 in fp32, zero in the bf16 hi plane
        assert row[n][0] == 1.0 and row[n][1] == np.float32(0.1), n
    for n in ("2^-25", "+2^-126", "+1e-30"):                            # zero in fp16
        assert row[n][0] == 1.0 and row[n][2] == np.float32(0.1), n
    for n in ("2^-134(1+2^-10)", "+2^-133"):                            # the smallest values that survive in bf16
        assert row[n][1] == 1.0, n
    for n in ("2^-25(1+2^-10)", "+2^-24"):                              # ... in fp16
        assert row[n][2] == 1.0, n
    for n in ("+0", "-0", "-2^-149", "-2^-126", "-2^-133", "-2^-24", "-1e-30", "-1e5", "-3e38"):
        assert row[n] == (np.float32(0.1),) * 3, n
    for n in ("65504", "+1e5", "+3e38"):                                # fp16 infinity is still 'positive and non-zero'
        assert row[n] == (1.0, 1.0, 1.0), n
    mag = np.abs(vals.astype(np.float64))
    assert np.array_equal(bf[mag >= 2.0 ** -133], f32[mag >= 2.0 ** -133])
    assert np.array_equal(fh[mag > 2.0 ** -25], f32[mag > 2.0 ** -25])
    assert D.BF16_AGREE >= 2.0 ** -133 and D.F16_AGREE > 2.0 ** -25      # the bounds asserted on the device lie inside the model's


def test_act_field_plants_every_special_at_the_listed_positions():
    shape, lo, hi = (1, 10, 14, 36), 5, 35
    act, where, special = D.act_field(shape, lo, hi, 'k')
    flat = act.reshape(-1, 36)
    assert D.edge_channels(36, lo, hi) == [4, 5, 34, 35]
    assert len(where) == 4 * 2 * len(D.SPECIALS) and special.sum() == len(where)
    for px, c, i in where:
        assert flat[px, c].tobytes() == D.SPECIALS[i][1].tobytes()      # bit for bit: -0 and the denormals survive
    assert {px for px, _, i in where if i == 0} == {0, flat.shape[0] - 1}
    neg = (act[~special] < 0).mean()
    assert 0.45 < neg < 0.55 and np.abs(act[~special]).min() >= 0.5
    again = D.act_field(shape, lo, hi, 'k')[0]
    assert act.tobytes() == again.tobytes()


@pytest.mark.parametrize("N", [36, 40, 64, 128, 256, 388, 476, 512, 1028])
def test_ranges(N):
    rs = D.ranges(N)
    assert (0, N) in rs and (0, N // 2 // 4 * 4) in rs and (8, N - 8) in rs and (6, 7) in rs and (3, 9) in rs and (12, 12) in rs
    assert (N - 1, N) in rs and ((60, 70) in rs) == (N >= 70) and ((124, 132) in rs) == (N >= 132)
    lo, hi = D.straddle_range(N)
    assert lo % 4 == 1 and hi % 4 == 3 and 0 < lo < hi < N
    assert all(0 <= lo <= hi <= N for lo, hi in rs) and len(set(rs)) == len(rs)


def test_the_split_of_the_product_is_exact_and_the_product_differs():
    """10^6 multiples of 2^-18 below 2^4: fl32(s * 0.1f) splits into three bf16 planes exactly (expected_planes asserts it),
    differs from s wherever s != 0 — and from the product with 0.1 taken in double and rounded once (the last mutant)."""
    g = E.gen('products')
    s = (torch.randint(-2 ** 22 + 1, 2 ** 22, (10 ** 6,), generator=g).double() * 2.0 ** -18).numpy()
    s[:4] = [0.0, 2.0 ** -18, -(2.0 ** -18), 16 - 2.0 ** -18]
    slope = np.full(s.shape, D.TENTH)
    assert np.array_equal(D.expected(s[:, None], slope[:, None], 1, 1)[:, 0], s.astype(np.float32))      # empty range: s itself
    want = D.expected(s[:, None], slope[:, None], 0, 1)[:, 0]
    planes = D.expected_planes(want, 3)
    assert np.array_equal(planes.astype(np.float64).sum(0), want.astype(np.float64))
    assert np.all((want != s.astype(np.float32)) | (s == 0))
    once = (s * 0.1).astype(np.float32)                                 # 0.1 in double, one rounding
    n = int((once != want).sum())
    assert n > 1000, n
    with pytest.raises(AssertionError):
        D.assert_output(once[:, None], want[:, None], 1, F32_SENTINEL, "0.1 in double")
    h = D.expected_planes(want, 1, 4096.0)[0]
    assert np.array_equal(h, (want * np.float32(4096.0)).astype(np.float16).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("regime,case,deconv", D.problems(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_inputs_keep_the_multiply_visible(regime, case, deconv):
    """Both conditions for every (case, regime, range) the GPU tests run."""
    dz, w, ref, base = _problem(regime, case, deconv)
    N = case[3]
    s = base + ref
    names = [r[0] for r in D.ROWS if r[3] == case and r[4] == deconv]
    rs = D.ranges(N) if any(n not in D.BIG for n in names) else D.row_ranges(names[0], N)
    for lo, hi in rs:
        act = D.act_field(tuple(ref.shape), lo, hi, (regime, case))[0]
        D.assert_conditions(act, s, lo, hi, "%s %s [%d, %d)" % (regime, case, lo, hi))


# ------------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = [('lo', 'f32'), ('hi', 'f32'), ('quad', 'f32'), ('before', 'f32'), ('ge0', 'f32'), ('mid', 'planes'), ('ld', 'f32')]


@pytest.mark.parametrize("row", SMALL, ids=[r[0] for r in SMALL])
def test_wrong_epilogues_are_caught(row):
    name, entry, opts, case, deconv, P = row
    N = case[3]
    for regime in D.regimes(P, name):
        dz, w, ref, base = _problem(regime, case, deconv)
        kills = {m: [] for m, _ in MUTANTS}
        for lo, hi in D.ranges(N):
            act = D.act_field(tuple(ref.shape), lo, hi, (regime, case))[0]
            for source in ('f32', 'planes'):
                slope = D.slope_f32(act) if source == 'f32' else D.slope_bits(model_bits(act, P))
                want = D.expected(base + ref, slope, lo, hi)
                good = epilogue(base, ref, act, lo, hi, source, P)
                D.assert_output(good, want, N, F32_SENTINEL, "the right epilogue")
                for m, src in MUTANTS:
                    if src == source and caught(epilogue(base, ref, act, lo, hi, source, P, m), want, N):
                        kills[m].append((lo, hi))
        print(regime, {m: len(k) for m, k in kills.items()})
        rs = D.ranges(N)
        nonempty = [r for r in rs if r[1] > r[0]]
        for m in ('lo', 'hi'):                                          # a shifted end shows on EVERY range
            assert kills[m] == rs, (regime, m, kills[m])
        for m in ('before', 'ge0', 'mid', 'ld'):                        # ... these wherever something is multiplied
            assert kills[m] == nonempty, (regime, m, kills[m])
        assert kills['quad'] == [r for r in nonempty if r[0] % 4 or r[1] % 4], (regime, kills['quad'])


def test_comparators_see_leaks_and_stray_writes():
    g = E.gen('cmp')
    want = (E.ints((2, 3, 12), g, -5, 5) * 0.5).float().numpy()
    buf = np.full((2, 3, 16), F32_SENTINEL, dtype=np.float32)
    buf[..., :12] = want
    D.assert_output(buf, want, 12, F32_SENTINEL, "ok")
    for idx, v in (((1, 2, 12), 0.0), ((0, 0, 15), 2.0), ((1, 1, 3), np.nan), ((0, 2, 0), np.nextafter(buf[0, 2, 0], np.float32(9)))):
        b = buf.copy()
        b[idx] = np.float32(v)
        with pytest.raises(AssertionError, match="channel"):
            D.assert_output(b, want, 12, F32_SENTINEL, "bad")
    for P, scale in ((3, 0.0), (1, 4096.0)):
        vals = D.expected_planes(want, P, scale)
        bits = np.full((P, 2, 3, 32), D.SENTINEL, dtype=np.int16)
        model = torch.from_numpy(vals)
        enc = model.bfloat16().view(torch.int16).numpy() if P == 3 else model.half().view(torch.int16).numpy()
        bits[..., 4:9] = enc[..., 4:9]
        D.assert_planes(bits, vals, 4, 9, "ok")
        D.assert_planes(np.full_like(bits, D.SENTINEL), vals, 12, 12, "empty range")
        for idx, v in (((0, 1, 2, 3), 0), ((P - 1, 0, 0, 9), 0), ((0, 1, 1, 31), 0), ((P - 1, 1, 2, 6), D.SENTINEL),
                       ((0, 0, 1, 5), int(enc[0, 0, 1, 5]) ^ 1)):
            b = bits.copy()
            b[idx] = v
            with pytest.raises(AssertionError, match="planes"):
                D.assert_planes(b, vals, 4, 9, "bad")
