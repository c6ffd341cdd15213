"""tests/head_cases.py without a GPU: the table agrees with the dispatch mirror, every kernel form is reached, the exact-input problems
of every (case, regime) of tests/test_heads_gpu.py meet their conditions, and torch's plain fp32 CPU evaluation of every random-data
problem stays inside the bound the kernels are held to."""
import numpy as np
import pytest
import torch

import dgrad_epilogue as D
import exact_inputs as E
import head_cases as HC

REGIMES = ('dense', 'A3')


@pytest.mark.parametrize("c", HC.ALL, ids=lambda c: c.id)
def test_case_reaches_its_stated_form(c):
    got = HC.check_case(c)
    assert 'form' in c.facts and got['form'] in HC.FORMS
    if c.kind == 'head':
        B, H, W, Cin = c.shape
        assert Cin % 4 == 0 and c.Cout <= 4


def test_every_form_and_tail_is_reached():
    facts = {c.id: HC.facts_of(c) for c in HC.ALL}
    assert {f['form'] for f in facts.values()} == set(HC.FORMS)
    heads = [facts[c.id] for c in HC.HEADS]
    tile8 = [f for f in heads if f['form'] == 'tile8']
    strip4 = [f for f in heads if f['form'] == 'strip4']
    skinny = [f for f in heads if f['form'] == 'skinny']
    # the two sides of the threshold; ragged and whole last row tiles; partial, single-lane and whole quad groups
    assert any(f['npix'] == HC.TILE8_MIN_PIXELS for f in tile8) and any(HC.TILE8_MIN_PIXELS - 128 <= f['npix'] < HC.TILE8_MIN_PIXELS for f in strip4)
    assert {f['last_tile_rows'] for f in tile8} == {1, 2, 4}
    for group in (tile8, strip4):
        assert any(f['spw'] == 4 for f in group) and any(f['spw'] == 1 for f in group)
        assert any(f['groups'] > 1 and f['last_group_lanes'] == 1 for f in group) or any(f['last_group_lanes'] < 64 for f in group)
    assert any(f['spw'] == 4 and f['last_wave_strips'] < 4 and f['empty_waves'] for f in strip4)
    assert any(f['quads'] == 1 for f in strip4) and any(f['groups'] == 5 for f in strip4) and any(f['strips'] == 3 for f in strip4)
    assert any(f['fwd_passes'] == 2 for f in skinny) and any(f['dgrad_passes'] == 2 for f in skinny) and any(f['npix'] == 6 for f in skinny)
    assert {(c.Cout, c.k) for c in HC.TEMPLATES} == {(1, 3), (4, 3), (2, 1), (2, 5)}
    pw = [facts[c.id] for c in HC.POINTWISE]
    assert any(f['tail_strip'] for f in pw) and any(f['groups'] == 2 and f['last_group_lanes'] == 1 for f in pw) and any(f['quads'] == 1 for f in pw)
    tiny = [facts[c.id] for c in HC.TINY]
    assert any(f['npix'] == 1 for f in tiny) and any(f['wgrad_passes'] == 2 for f in tiny)
    assert any(f['fwd_passes'] == 2 and f['dgrad_passes'] == 1 for f in tiny) and any(f['dgrad_passes'] == 2 for f in tiny)
    # flow_wgrad_batched: one layer of each kind, and a batch without a plan
    assert [b[1] for b in HC.BATCH] == [0, 1, 2]
    for cid, kind, spw, blocks in HC.BATCH:
        c = HC.BY_ID[cid]
        assert HC.flow_wgrad_plan(HC.batch_kind(c), *c.shape[:3], c.shape[3] if c.kind == 'head' else 2) == (kind, spw, blocks)
    assert any(HC.flow_wgrad_plan('conv', *HC.BY_ID[i].shape) is None for i in HC.BATCH_FALLBACK)
    assert all(i in HC.BY_ID for i in HC.RANDOM_IDS) and {HC.BY_ID[i].facts['form'] for i in HC.RANDOM_IDS} == set(HC.FORMS)


def test_mirror_thresholds():
    assert HC.head_strip(1, 128, 128, 3, 2) == 8 and HC.head_strip(1, 127, 128, 3, 2) == 4 and HC.head_strip(4, 64, 68, 3, 2) == 4
    assert HC.head_strip(1, 128, 130, 3, 2) == 0 and HC.head_strip(1, 128, 128, 5, 2) == 0 and HC.head_strip(1, 128, 128, 3, 4) == 0
    assert HC.stream_grid(1) == 1 and HC.stream_grid(524288) == 2048 and HC.stream_grid(524289) == 2048 and HC.passes(524289, 2048) == 2
    assert HC.pointwise_form(32, 1, 1, 260, None) and not HC.pointwise_form(32, 1, 1, 257, None) and not HC.pointwise_form(32, 1, 1, 260, 257)
    assert not HC.pointwise_form(64, 1, 1, 260, None) and not HC.pointwise_form(32, 3, 1, 260, None)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("c", HC.ALL, ids=lambda c: c.id)
def test_exact_regime_conditions(c, regime):
    """The problem constructors assert E.assert_condition (sum |a b| + |bias| <= 2^21 granules, a non-zero exact fp32 result); the
    accumulating data gradient also needs |base + ref| exact and the conditions that keep the slope multiply visible."""
    case, deconv = HC.conv7(c), c.kind == 'tiny'
    B, H, W, Cin = case[:4]
    if c.kind != 'pointwise':
        E.conv_forward_problem(regime, *case, deconv=deconv)
    if c in HC.HEADS or deconv:
        E.conv_wgrad_problem(regime, *case, deconv=deconv)
    dz, w, ref = E.conv_dgrad_problem(regime, *case, deconv=deconv)
    base = E.ints((B, H, W, Cin), E.gen('base', regime, case), -3, 3) * E.GRANULE[regime]
    s = base + ref
    D.f32_exact(s)
    assert float(s.abs().max()) < 2.0 ** 22 * E.GRANULE[regime]
    if not deconv:
        hi = 2 if Cin == 4 else Cin // 2 // 4 * 4
        assert 0 < hi < Cin
        act = D.act_field((B, H, W, Cin), 0, hi, (regime, case))[0]
        D.assert_conditions(act, s, 0, hi, "%s %s" % (c.id, regime))


def _fp32_cpu(c, direction, p):
    """torch's plain fp32 CPU evaluation of a random-data problem."""
    B, H, W, Cin, Cout, k, stride = HC.conv7(c)
    deconv = c.kind == 'tiny'
    if direction == 'fwd':
        return [("forward", E._conv_ref(p['x'].float(), p['w'].float(), p['b'].float(), stride, deconv), p['v'], p['S'], p['n'])]
    if direction == 'wgrad':
        return [("filter gradient", E.wgrad_ref(p['x'].float(), p['dz'].float(), k, stride, deconv), p['v'], p['S'], p['n'])]
    x0 = torch.zeros(B, H, W, Cin, requires_grad=True)
    s = torch.autograd.grad(E._conv_ref(x0, p['w'].float(), None, stride, deconv), x0, p['dz'].float())[0]
    t = p['base'].float() + s
    hi = p['hi']
    slope = torch.where(p['act'].float() > 0, torch.tensor(1.0), torch.tensor(0.1))
    t[..., :hi] = t[..., :hi] * slope[..., :hi]
    return [("data gradient", s, p['v0'], p['S0'], p['n0']), ("data gradient, acc + slope", t, p['v'], p['S'], p['n'])]


@pytest.mark.parametrize("cid", HC.RANDOM_IDS)
def test_fp32_reference_stays_inside_the_bound(cid):
    """The bound of tests/test_heads_gpu.py (d) is a statement about fp32, not about the kernels: the reference alone meets it."""
    c = HC.BY_ID[cid]
    dirs = ('dgrad',) if c.kind == 'pointwise' else ('fwd', 'dgrad', 'wgrad')
    for direction in dirs:
        p = HC.random_problem(c, direction)
        for name in ('x', 'w', 'dz', 'base'):
            if name in p:                                                   # six decades, fp32 values
                a = p[name].abs()
                assert torch.equal(p[name], p[name].float().double()) and a.max() / a[a > 0].median() > 100
        for what, got, v, S, n in _fp32_cpu(c, direction, p):
            r = HC.bound_ratio(got.detach(), v, S, n)
            print("%-18s %-26s torch fp32 CPU: max |got - fp64| / bound = %.3g   (n = %d)" % (c.id, what, r, n))
            assert r <= 1.0, (cid, what, r)
    assert np.isfinite(r)
