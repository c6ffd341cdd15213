"""Ground-truth tracks and track scores without a GPU: the numpy definition of tests/track_score_ref.py — hand cases,
the coverage of its case set (asserted: the GPU test compares integers for equality, so every word has to be exercised by the
reference alone), mutants of the definition — and the C entry's declaration, workspace query and argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_ref as TR
import track_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.entry_cases()
BY_ID = dict(CASES)


@pytest.fixture(scope="module")
def lib():
    from unflow_amd import build, _lib
    build.build()
    L = _lib.lib()
    L.unflow_sequence_track_score_workspace_bytes.restype = ctypes.c_size_t
    return L


@pytest.fixture(scope="module")
def reference():
    """The reference's outputs of every case, computed once: {id: ({slot: (disp, alive, words, err)}, state)}."""
    return {cid: R.replay(c, c['gt_state']) for cid, c in CASES}


def _hand(kind='zero', nmaps=2, pattern='full', **kw):
    c = R.make_case('hand', anchors=1, kind=kind, nmaps=nmaps, pattern=pattern, noise=None, **dict(R.SMALL, **kw))
    N = c['N']
    c['gt_state'] = (np.zeros((N, 2), np.float32), np.ones(N, bool))
    c['pred_disp'][:] = 0
    c['pred_alive'][:] = True
    return c


# ------------------------------------------------------------------------------------------------- 1. hand cases
def test_zero_ground_truth_and_zero_prediction_are_all_within_with_no_error():
    c = _hand()
    outs, (disp, alive) = R.replay(c, c['gt_state'])
    assert sorted(outs) == [0, 1, 2]
    for i, (gd, ga, w, err) in outs.items():
        assert (gd == 0).all() and err == 0.0
        assert w[0] == w[2] == ga.sum() and w[1] == c['N'] == w[14] and w[15] == 0
        assert (w[3:8] == w[0]).all() and (w[8:13] == w[2]).all()
        assert w[13] == ga.sum()
    # the blobs of invalid and occluded pixels ended some tracks, for good
    assert 0 < outs[2][1].sum() < outs[0][1].sum() < c['N']
    assert not (outs[2][1] & ~outs[0][1]).any()


def test_an_offset_of_exactly_two_pixels_is_not_within_two_pixels():
    c = _hand()
    c['pred_disp'][..., 0] = 2.0
    outs, _ = R.replay(c, c['gt_state'])
    for i, (gd, ga, w, err) in outs.items():
        n = int(ga.sum())
        assert n > 0 and w[3] == 0 and w[4] == 0 and w[5] == n and w[8] == 0 and w[9] == 0 and w[10] == n      # d2 = 4: strict <
        assert err == 2.0 * n


def test_a_track_anchored_on_an_invalid_pixel_is_dead_after_slot_0():
    c = _hand(nmaps=1)
    c['gt_mask'][:, :, : c['h'], : c['w']] = 1.0
    x, y = 3, 2
    c['gt_mask'][0, 0, y, x] = 0.0
    n = y * c['w'] + x
    assert tuple(c['anchors'][n]) == (x, y)
    outs, (disp, alive) = R.replay(c, c['gt_state'])
    for i in (0, 1, 2):
        assert not outs[i][1][n] and outs[i][1].sum() == c['N'] - 1
        assert outs[i][2][13] == c['N'] - 1                   # the prediction says alive everywhere: one disagreement
    assert not alive[n]
    # with two maps the LAST map's mask decides: the same hole in map 0 alone is not seen, a hole in map 1 is
    c2 = _hand(nmaps=2)
    c2['gt_mask'][:, :, : c['h'], : c['w']] = 1.0
    c2['gt_mask'][0, 0, y, x] = 0.0
    assert R.replay(c2, c2['gt_state'])[0][0][1].all()
    c2['gt_mask'][1, 0, y, x] = 0.0
    assert not R.replay(c2, c2['gt_state'])[0][0][1][n]


def test_a_pair_without_ground_truth_ends_every_track():
    cid = 'ragged-S1-smooth-m2-full-m0@2'
    c = BY_ID[cid]
    outs, (disp, alive) = R.replay(c, c['gt_state'])
    assert outs[1][1].sum() > 100
    for i in (2, 3):
        assert not outs[i][1].any() and outs[i][2][0] == 0 and outs[i][2][2] == 0 and outs[i][3] == 0.0
        assert (outs[i][2][3:13] == 0).all()
        assert np.array_equal(outs[i][0].view(np.int32), outs[1][0].view(np.int32))       # ended where they were
    assert not alive.any()


def test_carry_source_zero_ignores_the_state():
    c = BY_ID['ragged-S1-smooth-m2-first']
    garbage = (np.full((c['N'], 2), np.nan, np.float32), np.zeros(c['N'], bool))
    a, b = R.replay(c, garbage), R.replay(c, c['gt_state'])
    for i in c['valid']:
        assert np.array_equal(a[0][i][0].view(np.int32), b[0][i][0].view(np.int32)) and np.array_equal(a[0][i][2], b[0][i][2])


# ------------------------------------------------------------------------------------------------- 2. coverage of the case set
def test_the_case_set_exercises_every_word(reference):
    words = np.stack([o[2] for outs, _ in reference.values() for o in outs.values()])
    assert (words[:, :14] > 0).any(axis=0).all(), "a word is zero in every case: %s" % np.flatnonzero(~(words[:, :14] > 0).any(axis=0))
    rising = [all(w[3 + k] < w[4 + k] for k in range(4)) for w in words]
    assert any(rising), "no slot has within_gt strictly rising through all five thresholds"
    big = [cid for cid, (outs, _) in reference.items() if any(o[2][2] >= 100 for o in outs.values())]
    assert len(big) >= 3, big
    assert (words[:, 15] == 0).all()
    # both kinds of disagreement, and both-alive tracks past the largest threshold, occur
    assert any(w[13] < w[14] for w in words) and any(w[12] < w[2] for w in words)
    # the shapes the kernel can go wrong at
    assert BY_ID['past-the-cap-smooth-m2-full']['N'] == 524365 > TR.GRID_CAP
    assert {c['nmaps'] for _, c in CASES} == {1, 2} and {c['pattern'] for _, c in CASES} == {'first', 'full', 'short', 'nopairs'}
    assert not BY_ID['ragged-S1-smooth-m2-nopairs']['valid']
    outside = BY_ID['sparse-65-smooth-m2-full']
    assert (outside['anchors'][:, 0] >= outside['w']).any()


def test_noise_spans_the_thresholds():
    c = BY_ID['ragged-S2-smooth-m2-full']
    outs, _ = R.replay(c, c['gt_state'])
    gd, ga, w, err = outs[1]
    d = np.sqrt(R.d2_of(c['pred_disp'][1], gd)[ga])
    assert d.min() < 0.4 and d.max() > 15 and d.max() < 20.5


# ------------------------------------------------------------------------------------------------- 3. mutants
def test_every_mutant_is_named():
    assert len(R.MUTANTS) >= 6 and len(set(R.MUTANTS)) == len(R.MUTANTS)


def _differs(a, b):
    for i in a[0]:
        if not (np.array_equal(a[0][i][1], b[0][i][1]) and np.array_equal(a[0][i][2], b[0][i][2]) and
                np.array_equal(a[0][i][0].view(np.int32), b[0][i][0].view(np.int32))):
            return True
    return not np.array_equal(a[1][1], b[1][1])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_a_mutant_of_the_definition_changes_a_case(mutant, reference):
    small = [(cid, c) for cid, c in CASES if c['N'] < 10000]
    changed = [cid for cid, c in small if _differs(R.replay(c, c['gt_state'], mutant=mutant), reference[cid])]
    print(mutant, "changes", changed)
    assert changed, mutant
    if mutant == 'le_threshold':          # what separates <= from <: a distance exactly on a threshold
        c = _hand()
        c['pred_disp'][..., 0] = 2.0
        assert _differs(R.replay(c, c['gt_state'], mutant=mutant), R.replay(c, c['gt_state']))


# ------------------------------------------------------------------------------------------------- 4. the C entry
def _declared(name, ret):
    txt = open(os.path.join(ROOT, "include", "unflow_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), txt)
    assert m, "%s is not declared in include/unflow_hip.h" % name
    return [a.strip() for a in m.group(1).split(',')]


def test_symbols_are_declared_and_exported(lib):
    args = _declared('unflow_sequence_track_score', 'int')
    assert len(args) == 18 and args[0] == 'const float* gt_flow' and args[1] == 'const float* gt_mask'
    assert args[2] == 'const int* tab' and args[-2] == 'void* workspace' and args[-1] == 'unflow_stream_t stream'
    assert _declared('unflow_sequence_track_score_workspace_bytes', 'size_t') == ['int B', 'int Ncap']
    assert hasattr(lib, 'unflow_sequence_track_score') and hasattr(lib, 'unflow_sequence_track_score_workspace_bytes')


def test_workspace_query(lib):
    q = lib.unflow_sequence_track_score_workspace_bytes
    # per slot a fp64 partial and 14 int32 partials for each of the 2048 blocks of the capped grid, and the ticket
    assert q(4, 1000) == 4 * 2048 * (8 + 14 * 4) + 16 and q(1, 1) == 2048 * 64 + 16
    assert q(4, 1000) % 8 == 0
    for B, Ncap in ((0, 10), (-1, 10), (4, 0), (4, -2), (513, 10)):
        assert q(B, Ncap) == 0, (B, Ncap)


def test_null_and_shape_errors_do_not_need_a_gpu(lib):
    n = ctypes.c_void_p(0)
    p = ctypes.c_void_p(256)                              # never dereferenced: every case below returns before a launch
    names = ('gt_flow', 'gt_mask', 'tab', 'B', 'Hmax', 'Wmax', 'anchors', 'Ncap', 'out_disp', 'out_alive', 'gt_disp', 'gt_alive',
             'out_gt_disp', 'out_gt_alive', 'scores', 'err', 'workspace')
    ok = dict({k: p for k in names}, B=2, Hmax=96, Wmax=160, anchors=n, Ncap=100)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.unflow_sequence_track_score(*[a[k] for k in names], n)
    for name in names:
        if name not in ('B', 'Hmax', 'Wmax', 'Ncap', 'anchors'):
            assert call(**{name: n}) == -1, name
    for name in ('B', 'Ncap', 'Hmax', 'Wmax'):
        assert call(**{name: 0}) == -5 and call(**{name: -3}) == -5, name
    assert call(Hmax=65536, Wmax=32768) == -5             # Hmax * Wmax = 2^31
    assert call(B=513) == -5                              # the block's LDS holds 512 slots
    assert call(anchors=p, B=0) == -5
