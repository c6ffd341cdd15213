"""The comparators and inputs of tests/test_plumbing_kernels_gpu.py proven without a GPU (tests/plumbing_parity.py): the fp32
torch-CPU evaluation of the oracle's expressions stands in for the kernels and must pass every assertion the GPU tests make
against the fp64 reference; the named mutants — a wrong partner, a wrong clamped tap, an unclamped x1, sign(0) = 1, the four
Adam faults, a dropped or doubled row of a bias sum, a wrong leaky-ReLU branch at +-0 / denormals — must fail them; the share
of pixels whose d_out the stage-input tests zero stays under its cap."""
import pytest
import torch

import loss_parity as L
import plumbing_parity as Q

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ stage input
@pytest.mark.parametrize("variant", Q.STAGE_VARIANTS)
@pytest.mark.parametrize("name,kind,shift", Q.STAGE_CASES)
def test_stage_input_fp32_oracle_passes(name, kind, shift, variant):
    r32, r64 = Q.ref_stage(name, kind, shift, variant, F32), Q.ref_stage(name, kind, shift, variant, F64)
    dout, share = Q.stage_dout(name, kind, shift, variant)
    assert share <= Q.NONSMOOTH_SHARE_CAP, share
    e_flow, o_flow, e_warp, o_warp = Q.check_stage_forward(r32['out'], r32, r64)
    assert (e_flow, e_warp) == (o_flow, o_warp) and max(o_flow, o_warp) < 1e-4
    e, own, bound = Q.check_stage_backward(r32['d_prev'], r32, r64)
    assert e == own and bound < 1e-3, (own, bound)           # the sensitivity the mutants below rely on
    print("stage %s/%s %s: zeroed share %.1e  fp32 oracle flow %.1e warp %.1e d_prev %.1e" % (name, kind, variant, share, o_flow,
                                                                                             o_warp, own))
    if name == 'BIG':
        return
    # the tap-by-tap transcription the mutants are applied to is the oracle, bit for bit forward
    first, second, prev, _ = Q.stage_operands(name, kind, shift, variant)
    s32 = Q.run_stage(Q.standin_stage(), first, second, prev, dout, F32)
    assert torch.equal(s32['out'], r32['out'])
    Q.check_stage_backward(s32['d_prev'], r32, r64)


def test_stage_input_operands():
    """Directed: second[n] = im[(n + shift) % N]; pair: the two halves as separate tensors; d_out differs from the raw draw only in
    channels 8..13 of the non-smooth pixels; the far sets clamp many taps; BIG is past one grid pass."""
    for name, kind, shift in Q.STAGE_CASES:
        inp = Q.make_stage_inputs(name, kind)
        N, H, W = inp['N'], inp['H'], inp['W']
        first, second, prev, raw = Q.stage_operands(name, kind, shift, 'directed')
        for n in range(N):
            assert torch.equal(second[n], inp['im'][(n + shift) % N])
        assert first.dtype == F32 and prev.dtype == F32 and tuple(prev.shape) == (N, inp['h'], inp['w'], 2)
        dout, share = Q.stage_dout(name, kind, shift, 'directed')
        changed = (dout != raw)
        assert not bool(changed[..., :8].any()) and abs(changed.any(3).float().mean().item() - share) < 1e-12
        if kind == 'far':
            flow = Q.ref_stage(name, kind, shift, 'directed', F64)['out'][..., 6:8]
            xs = torch.arange(W).view(1, 1, W) + flow[..., 0].floor()
            ys = torch.arange(H).view(1, H, 1) + flow[..., 1].floor()
            clamped = (xs < 0) | (xs + 1 > W - 1) | (ys < 0) | (ys + 1 > H - 1)
            assert clamped.float().mean().item() > (0.02 if name == 'BIG' else 0.2)
    N, H, W, _, _ = Q.STAGE_SHAPES['BIG']
    assert N * H * W > 2048 * 256
    assert {s for _, _, s in Q.STAGE_CASES if s not in (1,)} == {2, 3} and ('ODD', 'm4.0', 1) in Q.STAGE_CASES


def _stage_mutant(name, kind, shift, variant, mutant, shift_fault=0):
    first, second, prev, _ = Q.stage_operands(name, kind, shift + shift_fault, variant)
    dout, _ = Q.stage_dout(name, kind, shift, variant)
    return Q.run_stage(Q.standin_stage(mutant), first, second, prev, dout, F32)


@pytest.mark.parametrize("name,kind,shift,mutant", [('QUARTER', 'far', 3, 'partner'), ('ODD', 'm4.0', 1, 'partner'),
                                                    ('QUARTER', 'far', 3, 'tap'), ('BIG', 'far', 1, 'tap'),
                                                    ('QUARTER', 'far', 3, 'x1'), ('RAGGED', 'm1.5', 2, 'x1')])
def test_stage_input_mutants_fail(name, kind, shift, mutant):
    variant = 'directed'
    r32, r64 = Q.ref_stage(name, kind, shift, variant, F32), Q.ref_stage(name, kind, shift, variant, F64)
    if mutant == 'partner':
        bad = _stage_mutant(name, kind, shift, variant, None, shift_fault=1)       # (n + shift + 1) % N
    else:
        bad = _stage_mutant(name, kind, shift, variant, mutant)
    assert not torch.equal(bad['out'], r32['out'])
    with pytest.raises(AssertionError):
        Q.check_stage_forward(bad['out'], r32, r64)
    with pytest.raises(AssertionError):
        Q.check_stage_backward(bad['d_prev'], r32, r64)


@pytest.mark.parametrize("variant", Q.STAGE_VARIANTS)
def test_stage_input_sign_of_zero(variant):
    """The constructed pixels with warp == first exactly: the fp32 oracle (sign(0) = 0) passes with d_out kept whole, sign(0) = 1
    fails."""
    r32, r64 = Q.ref_kink(variant, F32), Q.ref_kink(variant, F64)
    zero = (r64['out'][..., 11:14] == 0).all(3)
    assert 0.4 < zero.float().mean().item() < 0.6 and torch.equal(zero, (r32['out'][..., 11:14] == 0).all(3))
    Q.check_stage_forward(r32['out'], r32, r64)
    Q.check_stage_backward(r32['d_prev'], r32, r64)
    ops = Q.kink_operands(variant)
    Q.check_stage_backward(Q.run_stage(Q.standin_stage(), *ops, F32)['d_prev'], r32, r64)
    with pytest.raises(AssertionError):
        Q.check_stage_backward(Q.run_stage(Q.standin_stage('sign0'), *ops, F32)['d_prev'], r32, r64)


def test_stage_input_prefilled_gradient_check_has_teeth():
    """The accumulate check (got - field against the reference, bound + PREFILL_EXTRA): a kernel that overwrites instead of adding,
    or adds twice, fails."""
    name, kind, shift = 'QUARTER', 'far', 3
    r32, r64 = Q.ref_stage(name, kind, shift, 'directed', F32), Q.ref_stage(name, kind, shift, 'directed', F64)
    field = torch.randn(r32['d_prev'].shape, generator=torch.Generator().manual_seed(1)) * r32['d_prev'].abs().max()
    Q.check_stage_backward((field + r32['d_prev']) - field, r32, r64, Q.PREFILL_EXTRA)
    for bad in (r32['d_prev'], field + 2 * r32['d_prev']):
        with pytest.raises(AssertionError):
            Q.check_stage_backward(bad - field, r32, r64, Q.PREFILL_EXTRA)


# ------------------------------------------------------------------------------------------------ Adam, L2, EPE
def test_adam_base_offsets_are_the_engines():
    """lo % 4 of every range part_buckets() yields for 'C' and 'CSS', with the default and a three-part cut, frozen and
    train_all."""
    from unflow_amd.core.engine import FlowNetEngine
    seen = set()
    for spec in ('C', 'CSS'):
        for extra in ({}, {'train_all': True}):
            eng = FlowNetEngine(1, 64, 64, params=dict(flownet=spec, **extra), device='cpu', layout_only=True, seed=None)
            for cut in (None, ('conv6', 'conv4')):
                if cut:
                    eng.set_backward_parts(cut)
                ranges = [r for part in eng.part_buckets() for r in part]
                assert ranges
                seen |= {lo % 4 for lo, _ in ranges}
    assert seen == set(Q.ADAM_LO_RESIDUES)
    assert {lo % 4 for lo in Q.ADAM_LOS} == seen and any(lo > 0 for lo in Q.ADAM_LOS)


@pytest.mark.parametrize("n", Q.ADAM_NS)
def test_adam_fp32_oracle_passes(n):
    inp = Q.make_adam_inputs(n)
    assert inp['m'].abs().max() > 0 and inp['v'].max() > 0                  # non-zero moments
    if n >= 5:
        z = (inp['m'] == 0) & (inp['v'] == 0)
        assert z.any() and all(bool((g[z] == 0).all()) for g in inp['g'])   # the 0 / (0 + eps) block
    regs = Q.adam_nregs(n)
    assert {0, n, n + 5, 4 * (n // 4) + 1} <= set(regs) and {s for _, s in Q.adam_cases(n)} == set(Q.ADAM_GSCALES)
    assert {r for r, _ in Q.adam_cases(n)} == set(regs)
    for n_reg, gscale in Q.adam_cases(n):
        r32, r64 = Q.ref_adam(n, n_reg, gscale, F32), Q.ref_adam(n, n_reg, gscale, F64)
        s32 = Q.standin_adam(n, n_reg, gscale) if n <= 4099 else None
        for i, t in enumerate(Q.ADAM_STEPS):
            Q.check_adam_step(r32[i], r32[i], r64[i], t)
            L.check_loss(r32[i]['loss'], r64[i]['loss'])
            assert not bool(torch.isnan(r64[i]['p']).any())
            if s32 is not None:                                            # the transcription the mutants are applied to is the oracle
                assert all(torch.equal(s32[i][k], r32[i][k]) for k in 'pmv')


@pytest.mark.parametrize("mutant", ['nreg', 'scale_after', 'eps_in', 'v_lin'])
def test_adam_mutants_fail(mutant):
    n, gscale = 1023, 0.5
    for n_reg in (1, 4 * (n // 4) + 1, n):          # inside the first float4, inside the tail, everything
        if mutant == 'nreg' and n_reg == n:
            continue                                # n + 1 regularises nothing more
        r32, r64 = Q.ref_adam(n, n_reg, gscale, F32), Q.ref_adam(n, n_reg, gscale, F64)
        bad = Q.standin_adam(n, n_reg, gscale, mutant)
        with pytest.raises(AssertionError):
            Q.check_adam_step(bad[0], r32[0], r64[0], 1)
        if mutant in ('nreg', 'scale_after'):       # the first moment alone sees these two, on a single element
            bound, _ = L.grad_bound(r32[0]['m'], r64[0]['m'], floor=Q.MOMENT_FLOOR)
            with pytest.raises(AssertionError):
                L.check_grad(bad[0]['m'], r64[0]['m'], bound)
    # and the update comparator alone: one element one tenth of a step off
    r32, r64 = Q.ref_adam(n, n, 1.0, F32), Q.ref_adam(n, n, 1.0, F64)
    off = r32[0]['p'].clone()
    off[n - 1] += 0.1 * Q.adam_lr_t(1)
    with pytest.raises(AssertionError):
        Q.check_update(off, r32[0]['p'], r64[0]['p'], Q.adam_lr_t(1))
    nan = r32[0]['p'].clone()
    nan[0] = float('nan')
    with pytest.raises(AssertionError):
        Q.check_update(nan, r32[0]['p'], r64[0]['p'], Q.adam_lr_t(1))


def test_adam_from_zero_moments_is_blind_to_the_gradient_scale():
    """Why the inputs start from non-zero moments: from M = V = 0 the first update is lr * sign(g) whatever grad_scale is (an eighth
    of the gradient moves the step by 1 %, through eps)."""
    g = torch.tensor([3e-3, -2e-4], dtype=F64)
    ups = []
    for s in (1.0, 0.125):
        P, Mm, Vv = {'x': torch.zeros(2, dtype=F64)}, {'x': torch.zeros(2, dtype=F64)}, {'x': torch.zeros(2, dtype=F64)}
        Q.M.adam_step_tf(P, {'x': g * s}, Mm, Vv, 1, Q.ADAM_LR)
        ups.append(P['x'])
    assert (ups[0] - ups[1]).abs().max().item() < 2e-2 * Q.ADAM_LR


@pytest.mark.parametrize("n", Q.L2_NS)
def test_l2_fp32_passes(n):
    L.check_loss(Q.ref_l2(n, F32), Q.ref_l2(n, F64))
    p = Q.make_l2_input(n).double()
    dropped = 0.5 * Q.ADAM_L2 * float((p[:-3] ** 2).sum()) if n < 1000 else 0.5 * Q.ADAM_L2 * float((p[:-256] ** 2).sum())
    with pytest.raises(AssertionError):             # a lost tail (small n) / a lost block of 256 (2M)
        L.check_loss(dropped, Q.ref_l2(n, F64))


@pytest.mark.parametrize("npix", Q.EPE_NPIX)
def test_epe_sums_fp32_passes(npix):
    for masked in (False, True):
        for a, b in zip(Q.ref_epe(npix, masked, F32), Q.ref_epe(npix, masked, F64)):
            L.check_loss(a, b)
    assert Q.ref_epe(npix, False, F64)[1] == npix
    num, den = Q.ref_epe(npix, True, F64)
    assert 0 < den < npix and num > 0


# ------------------------------------------------------------------------------------------------ exact sums
def test_colsum_descriptors_cover_the_paths():
    D = Q.COLSUM_DESCS
    assert len(D) == 32
    assert {c for c, _, _, _ in D} == {2, 3, 64, 66, 68, 196, 1024}
    assert {p for _, _, p, _ in D} == {1, 17, 511, 512, 513, 1025, 131077}
    assert {Q.colsum_chunks(p) for _, _, p, _ in D} == {1, 2, 256}
    assert 131077 % 256 != 0 and 1025 % 2 != 0                                           # ragged last chunks
    paths = [Q.colsum_path(c, c + pad, off) for c, pad, _, off in D]
    assert paths[0] == paths[-1] == 'scalar' and paths.count('vec') >= 12 and paths.count('scalar') >= 12
    assert any(pad == 2 and c % 4 == 0 for c, pad, _, _ in D)                              # ld = C + 2: scalar by the pitch
    assert any(off == 1 and c % 4 == 0 and pad % 4 == 0 for c, pad, _, off in D)           # scalar by the pointer alone
    assert any(pad == 4 and c % 4 == 0 and off == 0 and p == 131077 for c, pad, p, off in D)   # vector path, 256 chunks
    assert [paths[i] for i in Q.COLSUM_SINGLES] == ['scalar', 'vec', 'vec', 'scalar']
    assert [Q.colsum_chunks(D[i][2]) for i in Q.COLSUM_SINGLES] == [256, 2, 256, 256]
    assert sum(p * (c + pad) for c, pad, p, _ in D) * 4 < 400e6                            # bytes of one launch's inputs


@pytest.mark.parametrize("i", [0, 6, 8, 12, 31])
def test_colsum_inputs_are_exact_and_sensitive(i):
    x, want = Q.make_colsum_input(i)
    C = Q.COLSUM_DESCS[i][0]
    assert x[:, :C].abs().max() <= 8 and 8 * x.shape[0] < 2 ** 24
    assert torch.equal(x[:, :C].sum(0), want)                                # fp32 partial sums in any order are exact
    assert torch.equal(x[:, :C].flip(0).cumsum(0)[-1], want)
    for bad in Q.colsum_wrong_rows(i):                                       # one row dropped, one row doubled
        assert not torch.equal(bad, want)


def test_leaky_gradient_inputs():
    dy, y, want = Q.make_leaky_inputs()
    npix, C, lddy, ldy = Q.LEAKY_SHAPE
    assert npix * C > 2048 * 256 > (npix - 1) * C and lddy != ldy and min(lddy, ldy) > C
    yv = y[:, :C]
    assert bool(((yv == 0) & torch.signbit(yv)).any()) and bool(((yv == 0) & ~torch.signbit(yv)).any())
    den = (yv != 0) & (yv.abs() < 1.17e-38)
    assert bool((den & (yv > 0)).any()) and bool((den & (yv < 0)).any())
    assert torch.equal(want[:, C:], dy[:, C:])
    ref64 = dy[:, :C].double() * torch.where(yv > 0, 1.0, float(torch.tensor(0.1, dtype=F32))).double()
    assert torch.equal(want[:, :C].double(), ref64.float().double())        # the fp32 product, correctly rounded
    # wrong branches: ties to the 1-branch; denormals flushed to zero
    for slope in (torch.where(yv >= 0, 1.0, 0.1), torch.where(yv > 1.17e-38, 1.0, 0.1)):
        assert not torch.equal(dy[:, :C] * slope.float(), want[:, :C])


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("name", list(Q.RESIZE_CASES))
def test_resize_fp32_oracle_passes(name):
    r32 = Q.ref_resize(name, F32)
    worst, own, bound = Q.check_resize(r32, name)
    assert worst == own and bound < 1e-5
    (B, H, W, C), (oh, ow), _ = Q.RESIZE_CASES[name]
    assert tuple(r32.shape) == (B, oh, ow, C)
    bad = r32.clone()
    bad[-1, -1, -1, -1] += 1e-4 * r32.abs().max()
    with pytest.raises(AssertionError):
        Q.check_resize(bad, name)


def test_adam_hyperparameters_are_what_the_abi_carries():
    """beta travels as a float and the kernels form 1 - beta from it, as TF's fp32 ApplyAdam does: 1 - fl32(0.999) is 1.29e-5 below
    0.001.  The references therefore take the carried values (inputs are fp32 numbers, hyperparameters included): one fp64 step at
    the DECIMAL betas is further from the fp64 step at the carried ones than the whole update bound, on the elements whose V is
    small — a difference of the inputs, not of any kernel's arithmetic."""
    assert Q.ADAM_B1 == float(torch.tensor(0.9)) and Q.ADAM_B2 == float(torch.tensor(0.999)) and Q.ADAM_B2 != 0.999
    assert 1.2e-5 < 1 - (1 - Q.ADAM_B2) / 0.001 < 1.4e-5
    n = Q.ADAM_NS[-1]
    inp = Q.make_adam_inputs(n)
    ps = []
    for b1, b2 in ((0.9, 0.999), (Q.ADAM_B1, Q.ADAM_B2)):
        P, Mm, Vv = ({'x': inp[k].double().clone()} for k in 'pmv')
        Q.M.adam_step_tf(P, {'x': inp['g'][0].double()}, Mm, Vv, 1, Q.ADAM_LR, b1, b2, Q.ADAM_EPS)
        ps.append(P['x'])
    gap = ((ps[0] - ps[1]).abs().max() / Q.adam_lr_t(1)).item()
    r32, r64 = Q.ref_adam(n, 0, 1.0, F32), Q.ref_adam(n, 0, 1.0, F64)
    _, _, bound = Q.check_update(r32[0]['p'], r32[0]['p'], r64[0]['p'], Q.adam_lr_t(1))
    print("decimal vs carried betas, one fp64 step: %.2e of lr_t (update bound %.2e)" % (gap, bound))
    assert gap > bound
