"""-m gpu: unflow_sequence_track_score at its entry point on the cases of tests/track_score_ref.py.

1. its ground-truth tracks and final state against unflow_sequence_track — the existing kernel, already held to its mirror —
   launched on gt_flow[0] and the uint8 mask gt_mask[m - 1] == 0, bit for bit;
2. its integer words against the numpy scores of its OWN ground-truth tracks and the predictions it was given: equality;
3. err within 2^-22 relative of the fp64 sum of square roots of the same fp32 d2 (sqrtf: at most 1 ulp = 2^-23 relative per
   non-negative term; another 2^-23 for the fp64 summation order);
4. two launches and two graph replays: identical bytes;  5. sentinels, untouched slots and rows, scratch zero afterwards;
6. bad arguments write nothing;  7. a clip pushed 2, 3, 1, 1, 2 equals the clip pushed 3, 3, 3;  8. a NaN state is never read at
carry source 0."""
import ctypes

import numpy as np
import pytest
import torch

import track_score_ref as R

pytestmark = pytest.mark.gpu

CASES = R.entry_cases()
BY_ID = dict(CASES)
SENTINEL, SENTINEL_U8, SENTINEL_I32 = -777.0, 9, -12345
ERR_NULL, ERR_SHAPE = -1, -5
ERR_BOUND = 2.0 ** -22


def _L():
    from unflow_amd import _lib
    return _lib


class Launch:
    """The device buffers of one case, every output filled with a sentinel, and the call."""

    def __init__(self, case, state, dev, tab=None, pred=None):
        L = _L()
        self.case, self.dev = case, dev
        N, B = case['N'], case['B']
        self.Ncap = Ncap = case['Ncap']
        self.gt_flow = torch.from_numpy(case['gt_flow']).to(dev)
        self.gt_mask = torch.from_numpy(case['gt_mask']).to(dev)
        self.tab = torch.from_numpy(case['tab'] if tab is None else tab).to(dev)
        self.anchors = torch.from_numpy(case['anchors'].astype(np.int32)).to(dev) if case['sparse'] else None
        pd, pa = (case['pred_disp'], case['pred_alive']) if pred is None else pred
        self.out_disp = torch.full((B, Ncap, 2), SENTINEL, device=dev)
        self.out_alive = torch.full((B, Ncap), SENTINEL_U8, dtype=torch.uint8, device=dev)
        self.out_disp[:, :N] = torch.from_numpy(pd).to(dev)
        self.out_alive[:, :N] = torch.from_numpy(pa.astype(np.uint8)).to(dev)
        self.disp = torch.full((Ncap, 2), SENTINEL, device=dev)
        self.alive = torch.full((Ncap,), SENTINEL_U8, dtype=torch.uint8, device=dev)
        if state is not None:
            self.disp[:N] = torch.from_numpy(state[0]).to(dev)
            self.alive[:N] = torch.from_numpy(state[1].astype(np.uint8)).to(dev)
        self.out_gt_disp = torch.full((B, Ncap, 2), SENTINEL, device=dev)
        self.out_gt_alive = torch.full((B, Ncap), SENTINEL_U8, dtype=torch.uint8, device=dev)
        # one guard row on either side of the scores and the error sums
        self.scores = torch.full((B + 2, 16), SENTINEL_I32, dtype=torch.int32, device=dev)
        self.err = torch.full((B + 2,), SENTINEL, dtype=torch.float64, device=dev)
        q = L.lib().unflow_sequence_track_score_workspace_bytes
        q.restype = ctypes.c_size_t
        self.ws_bytes = int(q(B, Ncap))
        assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
        self.ws = torch.zeros(self.ws_bytes // 8 + 2, dtype=torch.int64, device=dev)     # a guard word on either side
        self.ws[0] = self.ws[-1] = SENTINEL_I32

    def call(self, stream=None, **kw):
        L, c = _L(), self.case
        a = dict(B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], Ncap=self.Ncap)
        a.update(kw)
        return L.lib().unflow_sequence_track_score(
            L.ptr(self.gt_flow), L.ptr(self.gt_mask), L.ptr(self.tab), a['B'], a['Hmax'], a['Wmax'], L.ptr(self.anchors), a['Ncap'],
            L.ptr(self.out_disp), L.ptr(self.out_alive), L.ptr(self.disp), L.ptr(self.alive), L.ptr(self.out_gt_disp),
            L.ptr(self.out_gt_alive), L.ptr(self.scores[1:]), L.ptr(self.err[1:]), L.ptr(self.ws[1:]),
            L.stream() if stream is None else stream)

    def run(self, **kw):
        st = self.call(**kw)
        torch.cuda.synchronize()
        return st

    def outputs(self):
        return [t.clone() for t in (self.out_gt_disp, self.out_gt_alive, self.disp, self.alive, self.scores, self.err)]

    def untouched(self):
        return bool((self.out_gt_disp == SENTINEL).all()) and bool((self.out_gt_alive == SENTINEL_U8).all()) and \
            bool((self.scores == SENTINEL_I32).all()) and bool((self.err == SENTINEL).all()) and self.scratch_clean()

    def scratch_clean(self):
        return bool((self.ws[1:-1] == 0).all()) and int(self.ws[0]) == SENTINEL_I32 and int(self.ws[-1]) == SENTINEL_I32

    def results(self):
        """({valid slot: (gt disp, gt alive, words, err)}, the state); checks everything a launch must leave alone (5)."""
        c, N = self.case, self.case['N']
        od, oa = self.out_gt_disp.cpu().numpy(), self.out_gt_alive.cpu().numpy()
        sd, sa = self.disp.cpu().numpy(), self.alive.cpu().numpy()
        sc, er = self.scores.cpu().numpy(), self.err.cpu().numpy()
        assert self.scratch_clean(), "the scratch is not zero after the launch"
        assert (sc[0] == SENTINEL_I32).all() and (sc[-1] == SENTINEL_I32).all() and er[0] == SENTINEL and er[-1] == SENTINEL
        for i in range(c['B']):
            if i not in c['valid']:
                assert (od[i] == SENTINEL).all() and (oa[i] == SENTINEL_U8).all(), "slot %d is no pair and was written" % i
                assert (sc[1 + i] == SENTINEL_I32).all() and er[1 + i] == SENTINEL, "slot %d is no pair and was scored" % i
        assert (od[:, N:] == SENTINEL).all() and (oa[:, N:] == SENTINEL_U8).all(), "rows beyond the tracks were written"
        assert (sd[N:] == SENTINEL).all() and (sa[N:] == SENTINEL_U8).all(), "state beyond the tracks was written"
        if c['valid']:
            assert set(np.unique(oa[list(c['valid']), :N])) <= {0, 1} and set(np.unique(sa[:N])) <= {0, 1}
        outs = {i: (od[i, :N].copy(), oa[i, :N].astype(bool), sc[1 + i].copy(), float(er[1 + i])) for i in c['valid']}
        return outs, (sd[:N].copy(), sa[:N])


def _track_kernel(case, state, dev):
    """unflow_sequence_track on gt_flow[0] and the uint8 mask of every slot: ({slot: (disp, alive)}, state).  A slot without
    ground truth (m = 0) ends every track: a mask of ones."""
    L = _L()
    N, B, Ncap = case['N'], case['B'], case['Ncap']
    occ = np.ones(case['gt_mask'].shape[1:], np.uint8)
    for i, m in case['nmaps_of'].items():
        if m > 0:
            occ[i] = R.occ_of(case['gt_mask'], m, i)
    flow, occ = torch.from_numpy(case['gt_flow'][0]).to(dev), torch.from_numpy(occ).to(dev)
    tab = torch.from_numpy(case['tab']).to(dev)
    anchors = torch.from_numpy(case['anchors'].astype(np.int32)).to(dev) if case['sparse'] else None
    disp, alive = torch.zeros(Ncap, 2, device=dev), torch.zeros(Ncap, dtype=torch.uint8, device=dev)
    if state is not None:
        disp[:N], alive[:N] = torch.from_numpy(state[0]).to(dev), torch.from_numpy(state[1].astype(np.uint8)).to(dev)
    od, oa = torch.zeros(B, Ncap, 2, device=dev), torch.zeros(B, Ncap, dtype=torch.uint8, device=dev)
    assert L.lib().unflow_sequence_track(L.ptr(flow), L.ptr(occ), L.ptr(tab), B, case['Hmax'], case['Wmax'], L.ptr(anchors), Ncap,
                                         L.ptr(disp), L.ptr(alive), L.ptr(od), L.ptr(oa), L.stream()) == 0
    torch.cuda.synchronize()
    od, oa = od.cpu().numpy(), oa.cpu().numpy()
    return {i: (od[i, :N], oa[i, :N].astype(bool)) for i in case['valid']}, (disp.cpu().numpy()[:N], alive.cpu().numpy()[:N])


def _bits(a):
    return a.view(np.int32)


def _check(case, outs, state, want, want_state, pred=None):
    """Checks 1 to 3 of one launch; returns the worst ratio of err's error to its bound."""
    pd, pa = (case['pred_disp'], case['pred_alive']) if pred is None else pred
    worst = 0.0
    assert sorted(outs) == list(case['valid'])
    for i in case['valid']:
        gd, ga, words, err = outs[i]
        assert np.array_equal(_bits(gd), _bits(want[i][0])), "slot %d: the ground-truth displacements differ" % i       # 1
        assert np.array_equal(ga, want[i][1]), "slot %d: the ground-truth alive flags differ" % i
        ref_words, _ = R.score(pd[i], pa[i], gd, ga)                                                                    # 2
        assert np.array_equal(words, ref_words), ("slot %d" % i, words, ref_words)
        exact = R.err_exact(pd[i], pa[i], gd, ga)                                                                        # 3
        if np.isfinite(exact):
            assert abs(err - exact) <= ERR_BOUND * exact, ("slot %d" % i, err, exact)
            worst = max(worst, abs(err - exact) / (ERR_BOUND * exact) if exact else 0.0)
        else:
            assert np.isnan(err) == np.isnan(exact) and (np.isnan(exact) or err == exact)
    assert np.array_equal(_bits(state[0]), _bits(want_state[0])) and np.array_equal(state[1].astype(bool), want_state[1].astype(bool))
    return worst


# ------------------------------------------------------------------------------------------------- 1, 2, 3, 5
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_ground_truth_tracks_words_and_error_sum(cid, dev):
    case = BY_ID[cid]
    state = case['gt_state'] if case['carry'] else None           # carry source 0: the state holds the sentinel, never read
    run = Launch(case, state, dev)
    assert run.run() == 0
    outs, new_state = run.results()
    want, want_state = _track_kernel(case, state, dev)
    if not case['valid'] and not case['carry']:                   # no pair: both kernels initialise the state and stop
        assert (new_state[0] == 0).all() and new_state[1].all()
    worst = _check(case, outs, new_state, want, want_state)
    print("%s: N = %d, valid %s, n_gt / n_pred / n_both %s, err error / bound %.3f"
          % (cid, case['N'], case['valid'], [tuple(int(v) for v in o[2][:3]) for o in outs.values()], worst))


# ------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("cid", ['ragged-S1-smooth-m2-first', 'past-the-cap-smooth-m2-full'])
def test_launches_and_graph_replays_give_identical_bytes(cid, dev):
    case = BY_ID[cid]
    state = case['gt_state'] if case['carry'] else None
    runs = [Launch(case, state, dev) for _ in range(4)]
    assert runs[0].run() == 0 and runs[1].run() == 0
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    graphs = []
    for r in runs[2:]:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):          # captured, not run: the state is still the case's
                assert r.call(stream=ctypes.c_void_p(s.cuda_stream)) == 0
        graphs.append(g)
    torch.cuda.current_stream(dev).wait_stream(s)
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    ref = runs[0].outputs()
    for r in runs:
        r.results()
        for a, b in zip(ref, r.outputs()):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert float(ref[5][1 + case['valid'][0]]) > 0


# ------------------------------------------------------------------------------------------------- 6
def test_bad_arguments_write_nothing(dev):
    case = BY_ID['ragged-S2-smooth-m2-full']
    run = Launch(case, case['gt_state'], dev)
    before = (run.disp.clone(), run.alive.clone())
    for kw in (dict(B=0), dict(B=-1), dict(B=513), dict(Ncap=0), dict(Ncap=-5), dict(Hmax=0), dict(Wmax=-1),
               dict(Hmax=65536, Wmax=32768)):
        assert run.run(**kw) == ERR_SHAPE, kw
    L = _L()
    null = L.lib().unflow_sequence_track_score(None, L.ptr(run.gt_mask), L.ptr(run.tab), case['B'], case['Hmax'], case['Wmax'], None,
                                               run.Ncap, L.ptr(run.out_disp), L.ptr(run.out_alive), L.ptr(run.disp),
                                               L.ptr(run.alive), L.ptr(run.out_gt_disp), L.ptr(run.out_gt_alive),
                                               L.ptr(run.scores[1:]), L.ptr(run.err[1:]), L.ptr(run.ws[1:]), L.stream())
    torch.cuda.synchronize()
    assert null == ERR_NULL
    assert run.untouched() and torch.equal(run.disp, before[0]) and torch.equal(run.alive, before[1])
    # a dense grid of stride 0 or less is read on the device: the launch succeeds, tracks nothing and scores nothing
    for S in (0, -3):
        tab = case['tab'].copy()
        tab[16 * case['B'] + 2] = S
        bad = Launch(case, case['gt_state'], dev, tab=tab)
        assert bad.run() == 0
        assert bad.untouched() and torch.equal(bad.disp, before[0]) and torch.equal(bad.alive, before[1])
    # a pair slot whose frame exceeds the buffers is no pair
    tab = case['tab'].copy()
    tab[8 * case['B'] + 1] = case['Wmax'] + 1
    odd = Launch(dict(case, valid=[1, 2, 3]), case['gt_state'], dev, tab=tab)
    assert odd.run() == 0
    odd.results()
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 7
def test_uneven_pushes_through_one_state_equal_even_ones(dev):
    """Nine frames (eight pairs) of one clip through one device state, pushed 2, 3, 1, 1, 2 and pushed 3, 3, 3: the same
    ground-truth tracks, words and error sums per pair, and the same final state."""
    from unflow_amd.core.inference import sequence_tables
    B, shape = 3, dict(R.RAGGED, B=8)
    clip = R.make_case('clip', anchors=1, kind='smooth', nmaps=2, pattern='full', **shape)      # slot p: pair (p, p + 1)
    h, w, N = clip['h'], clip['w'], clip['N']

    def pushed(pushes):
        state, carry, n0, got = None, 0, 0, {}
        for k in pushes:
            tab, valid, nxt = sequence_tables((h, w), k, B, carry, track=(1, N), nmaps=2)
            # pair slot i of this push ends at frame n0 + i: clip pair n0 + i - 1
            src = [n0 + i - 1 for i in range(B)]
            take = lambda a: np.stack([a[:, p] if 0 <= p < 8 and i in valid else np.zeros_like(a[:, 0])      # noqa: E731
                                       for i, p in enumerate(src)], axis=1)
            pred = (np.stack([clip['pred_disp'][p] if i in valid else np.zeros((N, 2), np.float32) for i, p in enumerate(src)]),
                    np.stack([clip['pred_alive'][p] if i in valid else np.zeros(N, bool) for i, p in enumerate(src)]))
            part = dict(clip, B=B, carry=carry, valid=valid, tab=tab, gt_flow=take(clip['gt_flow']), gt_mask=take(clip['gt_mask']),
                        nmaps_of={i: 2 for i in valid})
            run = Launch(part, state, dev, pred=pred)
            assert run.run() == 0
            outs, state = run.results()
            state = (state[0], state[1].astype(bool))
            got.update({src[i]: outs[i] for i in valid})
            carry, n0 = nxt, n0 + k
        assert n0 == 9 and sorted(got) == list(range(8))
        return got, state
    a, sa = pushed((2, 3, 1, 1, 2))
    b, sb = pushed((3, 3, 3))
    for p in range(8):
        assert np.array_equal(_bits(a[p][0]), _bits(b[p][0])) and np.array_equal(a[p][1], b[p][1]), p
        assert np.array_equal(a[p][2], b[p][2]) and a[p][3] == b[p][3], p
    assert np.array_equal(_bits(sa[0]), _bits(sb[0])) and np.array_equal(sa[1], sb[1])
    assert 0 < a[7][1].sum() < a[0][1].sum() and a[7][2][2] >= 100          # tracks die along the clip; many live to its end


# ------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("cid", ['ragged-S1-smooth-m2-first', 'ragged-S1-smooth-m2-nopairs'])
def test_a_nan_state_is_never_read_at_carry_source_zero(cid, dev):
    case = BY_ID[cid]
    assert case['carry'] == 0
    nan = (np.full((case['N'], 2), np.nan, np.float32), np.zeros(case['N'], bool))
    once, twice = Launch(case, nan, dev), Launch(case, None, dev)
    assert once.run() == 0 and twice.run() == 0 and twice.run() == 0        # the eager pass and the first replay: one run
    a, b = once.results(), twice.results()
    for i in case['valid']:
        assert np.array_equal(_bits(a[0][i][0]), _bits(b[0][i][0])) and np.array_equal(a[0][i][2], b[0][i][2])
        assert np.isfinite(a[0][i][0]).all() and a[0][i][3] == b[0][i][3]
    assert np.isfinite(a[1][0]).all() and np.array_equal(_bits(a[1][0]), _bits(b[1][0]))
