"""The definition of unflow_sequence_track_score (include/unflow_hip.h) in numpy, its cases and synthetic inputs, for
tests/test_track_score_cpu.py (which proves it without a GPU) and tests/test_track_score_gpu.py.  Not a test file.

The ground-truth step IS tests/track_ref.py's step — unflow_sequence_track's definition — behind a float-mask adaptor: the flow is
map 0 of the staged ground truth, the uint8 "occluded" mask is gt_mask[m - 1] == 0.  The scores are written with every fp32
operation as one numpy operation on float32 arrays, so each is rounded on its own, as the kernel rounds it."""
import functools

import numpy as np

import track_ref as TR
import warp_parity as WP

T = np.array([1, 4, 16, 64, 256], np.float32)          # squared thresholds: 1, 2, 4, 8, 16 px
WORDS = 16
MUTANTS = ('flow_map1', 'mask_map0', 'le_threshold', 'dead_pred_out', 'reinit', 'pitch_w')


def occ_of(gt_mask, m, i, mutant=None):
    """The float-mask adaptor: the uint8 mask track_ref.step takes, 1 where slot i's ground truth ends a track.  Mutant mask_map0:
    always map 0's mask (with two maps: the occlusions are not seen)."""
    k = 0 if mutant == 'mask_map0' else m - 1
    return (gt_mask[k][i] == 0).astype(np.uint8)


def gt_step(disp, alive, anchors, gt_flow, gt_mask, i, m, h, w, dt=np.float32, mutant=None):
    """One ground-truth step for pair slot i with m maps: (disp in dt, alive).  m < 1 ends every track.  Mutants: flow_map1 — the
    flow of the last map (zero under occlusions); pitch_w — track_ref's."""
    if m < 1:
        return disp.astype(dt), np.zeros_like(alive)
    flow = gt_flow[m - 1 if mutant == 'flow_map1' else 0][i]
    return TR.step(disp, alive, anchors, flow, occ_of(gt_mask, m, i, mutant), h, w, dt, 'pitch_w' if mutant == 'pitch_w' else None)


def d2_of(pred_disp, gt_disp):
    """The fp32 squared distance, each operation rounded on its own: two subtractions, two products, one sum."""
    assert pred_disp.dtype == np.float32 and gt_disp.dtype == np.float32
    with np.errstate(invalid='ignore', over='ignore'):
        du, dv = pred_disp[:, 0] - gt_disp[:, 0], pred_disp[:, 1] - gt_disp[:, 1]
        uu, vv = du * du, dv * dv
        d2 = uu + vv
    assert d2.dtype == np.float32
    return d2


def score(pred_disp, pred_alive, gt_disp, gt_alive, mutant=None):
    """The 16 words of one slot and err, from N tracks' predicted and ground-truth (disp fp32 [N, 2], alive bool [N]).  err here is
    the fp64 sum of the fp32 square roots in index order (the kernel's order differs: tests allow for it).  Mutants: le_threshold
    — <= at the thresholds; dead_pred_out — within_gt counts only tracks whose prediction is alive."""
    N = len(gt_alive)
    d2 = d2_of(pred_disp, gt_disp)
    both = gt_alive & pred_alive
    with np.errstate(invalid='ignore'):
        near = [(d2 <= t) if mutant == 'le_threshold' else (d2 < t) for t in T]        # a NaN compares false
    words = np.zeros(WORDS, np.int32)
    words[0], words[1], words[2] = gt_alive.sum(), pred_alive.sum(), both.sum()
    base = both if mutant == 'dead_pred_out' else gt_alive
    for k in range(5):
        words[3 + k] = (base & near[k]).sum()
        words[8 + k] = (both & near[k]).sum()
    words[13] = (gt_alive == pred_alive).sum()
    words[14] = N
    with np.errstate(invalid='ignore'):
        err = float(np.sqrt(d2[both]).astype(np.float64).sum())
    return words, err


def err_exact(pred_disp, pred_alive, gt_disp, gt_alive):
    """The yardstick of err: the sum of the fp64 square roots of the same fp32 d2, and the sum of their magnitudes (= itself: the
    terms are non-negative) — what the kernel's sqrtf (at most 1 ulp = 2^-23 relative per term) and fp64 summation are held to."""
    d2 = d2_of(pred_disp, gt_disp)[gt_alive & pred_alive].astype(np.float64)
    with np.errstate(invalid='ignore'):
        return float(np.sqrt(d2).sum())


def replay(case, state, dt=np.float32, mutant=None):
    """One launch on `case` from state (gt disp [N, 2] fp32, gt alive [N] bool): ({slot: (gt disp fp32, gt alive, words, err)} of
    the valid slots, the new state).  Mutant reinit: the state is re-initialised on every launch, whatever the carry source."""
    N = case['N']
    if case['carry'] == 0 or mutant == 'reinit':
        disp, alive = np.zeros((N, 2), np.float32), np.ones(N, bool)
    else:
        disp, alive = state[0].copy(), state[1].copy()
    outs = {}
    for i in case['valid']:
        new, alive = gt_step(disp, alive, case['anchors'], case['gt_flow'], case['gt_mask'], i, case['nmaps_of'][i], case['h'],
                             case['w'], dt, mutant)
        with np.errstate(invalid='ignore', over='ignore'):
            disp = new.astype(np.float32)
        words, err = score(case['pred_disp'][i], case['pred_alive'][i], disp, alive, mutant)
        outs[i] = (disp, alive, words, err)
    return outs, (disp, alive)


# ------------------------------------------------------------------------------------------------- inputs
def draw_gt(rs, B, Hmax, Wmax, h, w, kind):
    """gt_flow [2, B, Hmax, Wmax, 2] and gt_mask [2, B, Hmax, Wmax] fp32 in the staged layout of a two-map ground truth: map 0 the
    full flow and the valid pixels (a blob of invalid ones per slot), map 1 the non-occluded ones (a second blob occluded) with
    its flow zeroed under them.  Outside (h, w): NaN flow and mask 0 — never to be read."""
    flow = TR.draw_flows(rs, B, Hmax, Wmax, h, w, kind)
    invalid, occluded = TR.draw_occ(rs, B, Hmax, Wmax, h, w), TR.draw_occ(rs, B, Hmax, Wmax, h, w)
    m0 = (invalid == 0).astype(np.float32)
    m1 = m0 * (occluded == 0).astype(np.float32)
    with np.errstate(invalid='ignore'):
        f1 = np.where(m1[..., None] > 0, flow, np.float32(0)).astype(np.float32)
    f1[:, h:] = np.nan
    f1[:, :, w:] = np.nan
    return np.stack([flow, f1]), np.stack([m0, m1])


def make_case(name, B, Hmax, Wmax, h, w, anchors, kind, nmaps, pattern, noise=(0.3, 20.0), m0_slot=None, seed=0, offset=None,
              poison_map1=False):
    """track_ref.make_case plus the staged ground truth, the table's nmaps words and a prediction per valid slot: the ground-truth
    track of the reference plus noise of a log-uniform magnitude in `noise` px (None: none) in a random direction, its alive flag
    the ground truth's flipped for one track in seven.  offset: instead of the noise, that exact (du, dv) for every track.  m0_slot:
    that slot's nmaps word is 0 (its pair has no ground truth).  poison_map1: map 1's flow, which the definition never reads, is
    NaN everywhere instead of map 0's zeroed under the occlusions (between those two the difference would never show: a tap
    under an occlusion either has weight zero or ends the track)."""
    from unflow_amd.core.inference import sequence_tables
    c = TR.make_case(name, B, Hmax, Wmax, h, w, anchors, kind, False, pattern, seed=seed)
    rs = WP._rs('track-score', name, kind, nmaps, pattern, seed)
    k, carry = TR.PATTERNS[pattern]
    k = B if k is None else k
    tab, valid, _ = sequence_tables((h, w), k, B, c['carry'], track=(c['S'], c['N']), nmaps=nmaps)
    assert valid == c['valid']
    nmaps_of = {i: nmaps for i in valid}
    if m0_slot is not None:
        assert m0_slot in valid
        tab[8 * B + 8 * m0_slot + 4] = 0
        nmaps_of[m0_slot] = 0
    gt_flow, gt_mask = draw_gt(rs, B, Hmax, Wmax, h, w, kind)
    if poison_map1:
        gt_flow[1] = np.nan
    c.update(tab=tab, nmaps=nmaps, nmaps_of=nmaps_of, gt_flow=gt_flow, gt_mask=gt_mask, gt_state=TR.draw_state(c),
             id='%s-%s-m%d-%s' % (name, kind, nmaps, pattern) + ('' if m0_slot is None else '-m0@%d' % m0_slot) +
             ('' if offset is None else '-exact') + ('-poison' if poison_map1 else ''))
    N = c['N']
    c['pred_disp'] = np.zeros((B, N, 2), np.float32)
    c['pred_alive'] = np.zeros((B, N), bool)
    chain, _ = replay(dict(c), c['gt_state'])
    for i in valid:
        gd, ga = chain[i][0], chain[i][1]
        if offset is not None:
            off = np.broadcast_to(np.asarray(offset, np.float64), (N, 2))
        elif noise is None:
            off = np.zeros((N, 2))
        else:
            mag = np.exp(rs.uniform(np.log(noise[0]), np.log(noise[1]), size=N))
            ang = rs.uniform(0, 2 * np.pi, size=N)
            off = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
        with np.errstate(invalid='ignore', over='ignore'):
            c['pred_disp'][i] = (gd.astype(np.float64) + off).astype(np.float32)
        c['pred_alive'][i] = ga ^ (rs.rand(N) < 1.0 / 7.0)
    return c


SMALL, RAGGED = TR.SMALL, TR.RAGGED
BIG_N = TR.GRID_CAP + 77                      # 524,365 tracks: past the 524,288 threads of the capped grid


@functools.lru_cache(maxsize=None)
def entry_cases():
    """(id, case): track_ref's small shapes — 9 x 11 around 7 x 10 with B = 3; 40 x 56 around 37 x 53 with B = 4 and S = 1, 2, 3;
    sparse N = 1 and N = 65 with an anchor outside; one- and two-map ground truth; first, short, full and no-pair replays; a pair
    without ground truth; and one launch past the grid's cap."""
    out = []
    for kind, nmaps in (('smooth', 2), ('const', 1), ('zero', 2), ('far', 2)):
        out.append(make_case('small', anchors=1, kind=kind, nmaps=nmaps, pattern='full', **SMALL))
    for nmaps, pattern in ((2, 'first'), (1, 'full'), (2, 'short'), (2, 'nopairs')):
        out.append(make_case('ragged-S1', anchors=1, kind='smooth', nmaps=nmaps, pattern=pattern, **RAGGED))
    out.append(make_case('ragged-S1', anchors=1, kind='tiny', nmaps=2, pattern='full', **RAGGED))
    for S in (2, 3):
        out.append(make_case('ragged-S%d' % S, anchors=S, kind='smooth', nmaps=2, pattern='full', poison_map1=S == 3, **RAGGED))
    # a distance exactly on a threshold: zero ground truth, every prediction 2 px off (d2 = 4 is not < 4)
    out.append(make_case('small', anchors=1, kind='zero', nmaps=1, pattern='full', offset=(2.0, 0.0), **SMALL))
    out.append(make_case('ragged-S1', anchors=1, kind='smooth', nmaps=2, pattern='full', m0_slot=2, **RAGGED))
    rs = WP._rs('track-score-points')
    for n in (1, 65):
        pts = TR.sparse_points(rs, n, RAGGED['h'], RAGGED['w'])
        out.append(make_case('sparse-%d' % n, anchors=pts, kind='smooth', nmaps=2, pattern='full', **RAGGED))
    big = TR.sparse_points(rs, BIG_N, RAGGED['h'], RAGGED['w'])
    out.append(make_case('past-the-cap', anchors=big, kind='smooth', nmaps=2, pattern='full', **dict(RAGGED, B=2)))
    return [(c['id'], c) for c in out]
