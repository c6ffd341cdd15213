"""-m gpu: held-out scores of the in-between frames — unflow_sequence_interpolate_score at its entry point against the
numpy definition of tests/mid_score_ref.py: the squared errors equal, the SSIM sums within a bound derived from the kernel's
summation shape; what it leaves alone, its scratch zero again; reproducibility between launches and graph replays; prev across
launches; and unflow_sequence_interpolate untouched by the entry that runs behind it."""
import numpy as np
import pytest
import torch

import mid_ref as M
import mid_score_ref as R

pytestmark = pytest.mark.gpu

CASES = R.entry_cases()
BY_ID = dict(CASES)
ERR_SHAPE, ERR_NULL = -5, -1
TAIL = 8


def _L():
    from unflow_amd import _lib
    return _lib


def _poison(shape, u8, dev):
    """A prev that must not be read: NaN (fp32) or a byte pattern."""
    return torch.full(shape, 0xEE, dtype=torch.uint8, device=dev) if u8 else torch.full(shape, float('nan'), device=dev)


class Launch:
    """The device buffers of one case, the outputs filled with sentinels (and a tail of rows behind them), and the call."""

    def __init__(self, case, prev, dev):
        L, c = _L(), case
        self.case, self.dev = case, dev
        n, B, Hm, Wm = c['n'], c['B'], c['Hmax'], c['Wmax']
        self.frames = torch.from_numpy(c['frames']).to(dev)
        self.tab = torch.from_numpy(c['tab']).to(dev)
        self.out_mid = torch.from_numpy(c['out_mid']).to(dev)
        self.truth = torch.from_numpy(c['truth']).to(dev)
        self.prev = _poison((Hm, Wm, 3), c['u8'], dev) if prev is None else torch.from_numpy(prev).to(dev)
        nbytes = int(L.lib().unflow_sequence_interpolate_score_workspace_bytes(n, B, Hm, Wm))
        assert nbytes > 0 and nbytes % 8 == 0
        self.ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
        self.words = n * B * 3
        self.out_sse = torch.full((self.words + TAIL,), R.SENTINEL_SSE, dtype=torch.int64, device=dev)
        self.out_ssim = torch.full((self.words + TAIL,), R.SENTINEL_SSIM, dtype=torch.float64, device=dev)

    def call(self, **kw):
        L, c = _L(), self.case
        a = dict(B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], n=c['n'], truth=self.truth)
        a.update(kw)
        return L.lib().unflow_sequence_interpolate_score(L.ptr(self.frames), L.ptr(self.tab), a['B'], a['Hmax'], a['Wmax'], a['n'],
                                                         L.ptr(self.out_mid), L.ptr(a['truth']), L.ptr(self.prev), L.ptr(self.ws),
                                                         L.ptr(self.out_sse), L.ptr(self.out_ssim), L.stream())

    def run(self, **kw):
        st = self.call(**kw)
        torch.cuda.synchronize()
        return st

    def reset(self):
        self.out_sse.fill_(R.SENTINEL_SSE)
        self.out_ssim.fill_(R.SENTINEL_SSIM)

    def outputs(self):
        """(out_sse, out_ssim) [n, B, 3] on the host; the tails behind them still hold the sentinels, the scratch is all zero."""
        c = self.case
        sse, ssim = self.out_sse.cpu().numpy(), self.out_ssim.cpu().numpy()
        assert (sse[self.words:] == R.SENTINEL_SSE).all() and (ssim[self.words:] == R.SENTINEL_SSIM).all(), "rows beyond B were written"
        assert not bool(self.ws.any()), "the scratch is not zero after the launch"
        return sse[:self.words].reshape(c['n'], c['B'], 3), ssim[:self.words].reshape(c['n'], c['B'], 3)

    def untouched(self):
        return bool((self.out_sse == R.SENTINEL_SSE).all()) and bool((self.out_ssim == R.SENTINEL_SSIM).all())


# ------------------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_kernel_equals_the_mirror(cid, dev):
    """Every case of mid_score_ref.entry_cases.  out_sse equals the mirror exactly.  out_ssim is within R.ssim_bound of the mirror's
    exactly rounded sum: every term carries at most 6 fp64 roundings of exact inputs (below 2^-50 relative, on terms of magnitude
    at most 1), and the kernel's fixed-order sum adds at most (longest serial chain + tree depth) * 2^-53 * sum |term|
    (R.sum_depth: a thread's 6 terms, the wave tree, the waves, the block's tiles, the last block's lane chain and tree).  Slots that
    are not scored and the rows behind the buffers keep their sentinels; the scratch is zero again; prev holds the last new
    frame's corner and nothing else changed in it."""
    case = BY_ID[cid]
    outs, new_prev = R.mirror_of(cid)
    run = Launch(case, R.prev_of(case), dev)               # carry source 0: a poisoned prev, never read
    before = run.prev.cpu().numpy()
    assert run.run() == 0
    worst = R.compare(case, outs, *run.outputs())
    h, w, k = case['h'], case['w'], case['k']
    after = run.prev.cpu().numpy()
    assert np.array_equal(after[:h, :w], case['frames'][k - 1, :h, :w], equal_nan=not case['u8'])
    assert np.array_equal(after[:h, :w], new_prev[:h, :w], equal_nan=not case['u8'])
    keep = np.ones(after.shape[:2], bool)
    keep[:h, :w] = False
    assert np.array_equal(after[keep], before[keep], equal_nan=not case['u8']), "prev was written outside the frame"
    print("%s: slots %s, depth %d, worst |ssim - fsum| / bound = %.3g" % (cid, case['scored'], R.sum_depth(case), worst))


def test_bad_arguments_write_nothing(dev):
    case = BY_ID['ragged-n3-u8-full-noise']
    run = Launch(case, R.prev_of(case), dev)
    before = run.prev.clone()
    for kw in (dict(n=0), dict(n=8), dict(n=-1), dict(B=0), dict(B=-2), dict(B=65536), dict(Hmax=0), dict(Wmax=-1),
               dict(Hmax=65536, Wmax=32768)):
        assert run.run(**kw) == ERR_SHAPE, kw
    assert run.run(truth=None) == ERR_NULL
    assert run.untouched() and torch.equal(run.prev, before) and not bool(run.ws.any())
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_two_graph_replays_give_identical_bytes(dev):
    """The pair past the block cap: every block sums several tiles and the last block of the slot is whichever comes last.  A
    second launch on the same buffers (the scratch left zero by the first; prev put back) and a captured graph replayed twice give
    the first launch's bytes."""
    case = BY_ID['past-the-cap-n1-u8-full-texture']
    eager = Launch(case, R.prev_of(case), dev)
    assert eager.run() == 0
    first = [t.copy() for t in eager.outputs()]
    eager.reset()
    eager.prev.copy_(torch.from_numpy(case['prev']))
    assert eager.run() == 0
    again = eager.outputs()
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    cap = Launch(case, R.prev_of(case), dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert cap.call() == 0
    torch.cuda.current_stream(dev).wait_stream(s)
    assert cap.untouched()                                # captured, not run
    for _ in range(2):
        cap.reset()
        cap.prev.copy_(torch.from_numpy(case['prev']))
        g.replay()
        torch.cuda.synchronize()
        got = cap.outputs()
        assert first[0].tobytes() == got[0].tobytes() and first[1].tobytes() == got[1].tobytes()


# ------------------------------------------------------------------------------------------------- 3. prev across launches
@pytest.mark.parametrize("u8,n", [(True, 1), (False, 3)], ids=['u8-n1', 'f32-n3'])
def test_a_clip_pushed_in_replays_of_different_lengths(u8, n, dev):
    """Nine network frames through B = 3 slots in pushes of 2, 3, 1, 1, 2: prev lives in ONE device buffer from launch to launch
    (poisoned before the first), the host overwrites the frames before each — every pair's scores are the mirror's, and those of
    the same clip pushed three at a time, bit for bit."""
    from unflow_amd.core.inference import sequence_tables
    shape = M.RAGGED
    B, Hm, Wm, h, w, T = shape['B'], shape['Hmax'], shape['Wmax'], shape['h'], shape['w'], 9
    rs = M.WP._rs('mid-score-clip', u8, n)
    clip = R.draw_clip(rs, T - 1, n, Hm, Wm, h, w, u8)
    net = clip[::n + 1]                                                    # the T network frames
    true = np.stack([clip[j::n + 1][:T - 1] for j in range(1, n + 1)])     # [n, T - 1]: frame j of pair p
    mids = np.clip(R.byte_of(true).astype(np.int64) + rs.randint(-9, 10, size=true.shape), 0, 255).astype(np.uint8)

    def pushed(pushes):
        got, carry, n0, dev_prev, host_prev = [], 0, 0, None, None
        for k in pushes:
            tab, valid, nxt = sequence_tables((h, w), k, B, carry, u8=u8, held=1)
            fr = np.full((B, Hm, Wm, 3), 77, clip.dtype)             # slots beyond the new frames: stale bytes
            fr[:k] = net[n0:n0 + k]
            idx = [min(max(n0 - 1 + i, 0), T - 2) for i in range(B)]        # pair slot i = pair n0 - 1 + i of the clip
            case = dict(B=B, Hmax=Hm, Wmax=Wm, h=h, w=w, n=n, u8=u8, k=k, carry=carry, tab=tab, valid=valid, scored=valid, frames=fr,
                        out_mid=np.ascontiguousarray(mids[:, idx]), truth=np.ascontiguousarray(true[:, idx]))
            run = Launch(case, None, dev)
            if dev_prev is not None:
                run.prev = dev_prev
            assert run.run() == 0
            outs, host_prev = R.replay(case, host_prev if carry else None)
            sse, ssim = run.outputs()
            R.compare(case, outs, sse, ssim)
            got += [(sse[:, i].copy(), ssim[:, i].copy()) for i in valid]
            dev_prev, carry, n0 = run.prev, nxt, n0 + k
        assert n0 == T and len(got) == T - 1
        return got
    ragged, whole = pushed((2, 3, 1, 1, 2)), pushed((3, 3, 3))
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(ragged, whole))
    assert all((a[0] > 0).all() for a in whole)


def test_carry_source_zero_never_reads_prev(dev):
    """Slot 0 marked a held pair in the table while the carry source is 0 (a table no estimator writes): it is no pair, and the NaN
    prev reaches nothing."""
    cid = 'ragged-n1-u8-first-texture'
    base = BY_ID[cid]
    case = R.make_case('ragged', n=3, u8=False, pattern='first', truth='texture', **M.RAGGED)
    assert case['carry'] == 0 and case['scored'] == [1, 2] and base['carry'] == 0
    tab = case['tab'].copy()
    B = case['B']
    tab[8 * B:8 * B + 8] = tab[8 * B + 8:8 * B + 16]
    run = Launch(dict(case, tab=tab), None, dev)
    assert bool(torch.isnan(run.prev).all()) and run.run() == 0
    R.compare(case, R.replay(case, None)[0], *run.outputs())


# ------------------------------------------------------------------------------------------------- 4. beside unflow_sequence_interpolate
def test_the_interpolation_is_unchanged_by_the_entry_behind_it(dev):
    """unflow_sequence_interpolate alone, and the same launch with the scores behind it on the same stream: out_mid, the hole
    counts and the interpolation's own prev are the same bytes; the scores are the mirror's on that out_mid."""
    L = _L()
    src = M.make_case('ragged', n=3, u8=True, bidir=False, kind='smooth', pattern='full', **M.RAGGED)
    n, B, Hm, Wm, h, w = src['n'], src['B'], src['Hmax'], src['Wmax'], src['h'], src['w']

    def interpolate(score):
        t = {k: torch.from_numpy(src[k]).to(dev) for k in ('frames', 'tab', 'flow_fw', 'prev')}
        sums = torch.zeros(int(L.lib().unflow_sequence_interpolate_workspace_bytes(n, B, Hm, Wm)) // 8, dtype=torch.int64, device=dev)
        mid = torch.full((n, B, Hm, Wm, 3), 0xA5, dtype=torch.uint8, device=dev)
        holes = torch.full((n, B), -777, dtype=torch.int32, device=dev)
        assert L.lib().unflow_sequence_interpolate(L.ptr(t['frames']), L.ptr(t['tab']), B, Hm, Wm, n, L.ptr(t['flow_fw']), None, None,
                                                   None, L.ptr(t['prev']), L.ptr(sums), L.ptr(mid), L.ptr(holes), L.stream()) == 0
        run = None
        if score:
            truth = np.ascontiguousarray(np.roll(src['frames'], 1, axis=2)[None].repeat(n, 0))
            tab = src['tab'].copy()
            tab[8 * B + 6:16 * B:8] = 1
            case = dict(src, tab=tab, scored=src['valid'], out_mid=None, truth=truth)
            run = Launch(dict(case, out_mid=np.zeros((1,), np.uint8)), src['prev'], dev)
            run.out_mid = mid
            assert run.call() == 0
        torch.cuda.synchronize()
        return mid.cpu().numpy(), holes.cpu().numpy(), t['prev'].cpu().numpy(), run
    alone, beside = interpolate(False), interpolate(True)
    assert all(np.array_equal(a, b) for a, b in zip(alone[:3], beside[:3]))
    run = beside[3]
    case = dict(run.case, out_mid=beside[0])
    R.compare(case, R.replay(case, src['prev'])[0], *run.outputs())
