"""GPU: .flo ground truth on the device — unflow_flo_to_flow_gt and unflow_sintel_gt (csrc/flo_decode.hip) against numpy, the
device readers of SintelInput / ChairsInput / MiddleburyInput against their host iterators, and the consumers
(FlowEstimator.evaluate / export / pictures, python -m unflow_amd.evaluate_flo) fed by either.  Every comparison of loader output
is exact and made on the int32 bit views of the float arrays, so -0 and NaN payloads count."""
import os
import threading

import numpy as np
import pytest
import torch

import flo_fixture as F
import png_cases as P
from unflow_amd import _lib
from unflow_amd.chairs.input import ChairsInput
from unflow_amd.core import input as I
from unflow_amd.core import png_device as D
from unflow_amd.middlebury.input import MiddleburyInput
from unflow_amd.sintel.input import SintelInput

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = -7.0
HS = WS = 16
SHAPES = [(11, 13), (16, 20), (5, 7)]


def loader_threads():
    return [t for t in threading.enumerate() if t.name.startswith(("png-producer", "png-inflate"))]


def window_of(img, oy, ox, Hs, Ws):
    """Output (y, x) = img[y + oy, x + ox] inside the file, 0 outside."""
    h, w = img.shape[:2]
    out = np.zeros((Hs, Ws) + img.shape[2:], dtype=img.dtype)
    y0, y1, x0, x1 = max(0, -oy), min(Hs, h - oy), max(0, -ox), min(Ws, w - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = img[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def origin(a):
    return D.window_origin(a.shape[0], HS), D.window_origin(a.shape[1], WS)


class Raw:
    """A raw buffer under construction: .flo bodies at chosen alignments and PNG scanline streams back to back."""

    def __init__(self):
        self.buf = bytearray()

    def put(self, data, align=1, skew=0):
        """Append `data` at the next offset that is `skew` behind a multiple of `align`; returns the offset."""
        while len(self.buf) % align != skew:
            self.buf.append(0xA5)
        off = len(self.buf)
        self.buf += bytes(data)
        return off

    def device(self):
        return torch.from_numpy(np.frombuffer(bytes(self.buf), dtype=np.uint8).copy()).to(DEV)


# ------------------------------------------------------------------------------------------------------------- kernels
def test_flo_to_flow_gt_against_numpy():
    rs = np.random.RandomState(30)
    flows = [F.flow_field(rs, h, w, special=0.3) for h, w in SHAPES]
    flows[0][0, 0] = (1e10, 1e10)                    # the first pixel inside the padded window, unknown
    flows[1][0, 2] = (np.float32(1e9), 0.0)          # exactly 1e9: not below
    flows[1][0, 3] = (np.nextafter(np.float32(1e9), np.float32(0)), -0.0)
    flows[2][4, 6] = (np.nan, np.inf)
    assert all(np.isin(F.bits(F.SPECIAL), F.bits(f)).all() for f in flows[:2])        # every special value occurs
    raw = Raw()
    offs = [raw.put(f.tobytes(), 16) for f in flows]
    off4 = raw.put(flows[2].tobytes(), 8, 4)         # a copy of file 2 at 4 (mod 8): the kernel's 4-byte loads
    assert off4 % 8 == 4
    # (file, src, origin): crop-or-pad of every file (11 x 13: pads both; 16 x 20: exact in y, crops x; 5 x 7: pads both), a crop
    # in x with padding in y in one entry, windows over a corner, a window entirely outside its file, and the 4-aligned copy
    entries = [(k, offs[k], origin(f)) for k, f in enumerate(flows)]
    entries += [(1, offs[1], (-3, 2)), (1, offs[1], (9, -5)), (0, offs[0], (-6, 4)), (0, offs[0], (100, 0)), (2, offs[2], (0, -16)),
                (2, off4, origin(flows[2])), (2, off4, (1, 2))]
    rows = [(src, 0) + flows[k].shape[:2] + (8, 4) + o for k, src, o in entries]
    n_raw = len(raw.buf)
    skipped = len(rows)
    rows.append((offs[0] + 2, 0, 11, 13, 8, 4, 0, 0))                      # src not a multiple of 4
    tall = (n_raw - offs[2]) // 56 + 1                                     # rows of 7 pairs: the last one runs past raw_bytes
    rows.append((offs[2], 0, tall, 7, 8, 4, 0, 0))
    rows.append((off4, 0, 5, 7, 8, 4, 0, 0)[:4] + (6, 2, 0, 0))            # a PNG row's bpp / sample_bytes
    rows.append((offs[0], 0, 11, 13, 8, 2, 0, 0))
    assert offs[2] + 56 * tall > n_raw >= offs[2] + 56 * (tall - 1)
    n = len(rows)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    flow = torch.full((n + 1, HS, WS, 2), CANARY, dtype=torch.float32, device=DEV)      # one slot more than the launch has entries
    mask = torch.full((n + 1, HS, WS), CANARY, dtype=torch.float32, device=DEV)
    raw_dev = raw.device()
    _lib.check(_lib.lib().unflow_flo_to_flow_gt(_lib.ptr(raw_dev), _lib.cl(n_raw), _lib.ptr(table), n, HS, WS, _lib.ptr(flow),
                                                _lib.ptr(mask), _lib.stream(DEV)), "flo_to_flow_gt")
    gf, gm = flow.cpu().numpy(), mask.cpu().numpy()
    for i, (k, _, (oy, ox)) in enumerate(entries):
        f = flows[k]
        with np.errstate(invalid='ignore'):
            known = ((f[..., 0] < np.float32(1e9)) & (f[..., 1] < np.float32(1e9))).astype(np.float32)
        assert F.same_bits(gf[i], window_of(f, oy, ox, HS, WS)), (i, k, oy, ox)
        assert F.same_bits(gm[i], window_of(known, oy, ox, HS, WS)), (i, k, oy, ox)
    assert (F.bits(gf[6]) == 0).all() and (gm[6] == 0).all()                # entirely outside: +0 and unknown
    assert gm[1][0, 0] == 0 and gm[1][0, 1] == 1                            # file 1 at ox = 2: exactly 1e9, then just below
    for i in range(skipped, n + 1):                                         # refused entries and the slot behind the launch
        assert (gf[i] == CANARY).all() and (gm[i] == CANARY).all(), "slot %d was written" % i
    # and the crop-or-pad entries are the host reader's maps
    inp = MiddleburyInput(None, 1, (HS, WS), normalize=False)
    for k, f in enumerate(flows):
        hf = inp._preprocess_map(f)
        assert F.same_bits(gf[k], hf)


MASK_KINDS = [(1, 8), (1, 16), (3, 8)]                 # (channels, depth): 8-bit grey, 16-bit grey, RGB


def mask_image(rs, h, w, ch, depth, p):
    """A mask PNG's samples: channel 0 is 0, 1 or 255 (16 bit: in the HIGH byte, under a random low byte — a sample of 0x00ff
    reads as 0), the other channels are random."""
    hit = rs.rand(h, w) < p
    top = np.asarray([1, 255])[rs.randint(0, 2, size=(h, w))] * hit
    img = P.random_image(rs, h, w, ch, depth)
    img[..., 0] = (top << 8) | rs.randint(0, 256, size=(h, w)) if depth == 16 else top
    return img, (top != 0).astype(np.float32)


def test_sintel_gt_against_numpy():
    rs = np.random.RandomState(31)
    n = len(SHAPES)
    flows, inv, occ = [], [], []
    for k, (h, w) in enumerate(SHAPES):
        f = F.flow_field(rs, h, w, special=0.2, values=[1e10, np.inf, np.nan, -0.0, 1e9])      # kept where the pixel is visible
        im_i, bit_i = mask_image(rs, h, w, *MASK_KINDS[k], p=0.25)
        im_o, bit_o = mask_image(rs, h, w, *MASK_KINDS[(k + 1) % 3], p=0.35)
        hidden = bit_o != 0
        f[hidden] = -np.abs(((rs.rand(int(hidden.sum()), 2) + 0.1) * 8).astype(np.float32))     # finite and negative under occlusion
        flows.append(f)
        inv.append((im_i, bit_i))
        occ.append((im_o, bit_o))
    raw = Raw()
    rows = [(raw.put(f.tobytes(), 16), 0) + f.shape[:2] + (8, 4) + origin(f) for f in flows]
    dst = 0
    for img, _ in inv + occ:                           # rows [n, 2n): invalid, [2n, 3n): occlusions — through the unfilter kernel
        b, depth, _, bpp = P.sample_bytes(img)
        stream = P.filter_rows(b, bpp, P.random_filters(rs, img.shape[0]))
        rows.append((raw.put(stream.tobytes()), dst) + img.shape[:2] + (bpp, depth // 8) + origin(img))
        dst += b.size
    rows.append((rows[0][0] + 1,) + rows[0][1:])       # a second launch's table: example 0 with a misaligned .flo row
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    raw_dev, n_raw = raw.device(), len(raw.buf)
    dec = torch.zeros(dst, dtype=torch.uint8, device=DEV)
    L = _lib.lib()
    _lib.check(L.unflow_png_unfilter(_lib.ptr(raw_dev), _lib.cl(n_raw), _lib.ptr(dec), _lib.cl(dst), _lib.ptr(table[n:]), 2 * n,
                                     _lib.stream(DEV)), "png_unfilter")
    flow = torch.full((2, n, HS, WS, 2), CANARY, dtype=torch.float32, device=DEV)
    mask = torch.full((2, n, HS, WS), CANARY, dtype=torch.float32, device=DEV)
    _lib.check(L.unflow_sintel_gt(_lib.ptr(raw_dev), _lib.cl(n_raw), _lib.ptr(dec), _lib.cl(dst), _lib.ptr(table), n, HS, WS,
                                  _lib.ptr(flow), _lib.ptr(mask), _lib.stream(DEV)), "sintel_gt")
    gf, gm = flow.cpu().numpy(), mask.cpu().numpy()
    signed_zero = 0
    for k, f in enumerate(flows):
        oy, ox = origin(f)
        fw = window_of(f, oy, ox, HS, WS)
        visible = 1 - window_of(occ[k][1], oy, ox, HS, WS)                  # padded first, composed afterwards
        valid = 1 - window_of(inv[k][1], oy, ox, HS, WS)
        assert F.same_bits(gf[0, k], fw) and F.same_bits(gf[1, k], fw * visible[:, :, None]), k
        assert F.same_bits(gm[0, k], valid) and F.same_bits(gm[1, k], valid * visible), k
        signed_zero += int((F.bits(gf[1, k]) == np.int32(-2 ** 31)).sum())
        outside = window_of(np.ones(f.shape[:2], np.float32), oy, ox, HS, WS) == 0
        if outside.any():
            assert (gm[:, k][:, outside] == 1).all() and (F.bits(gf[:, k][:, outside]) == 0).all()
    assert signed_zero > 20
    visible_nan = [np.isnan(gf[1, k]) & (window_of(occ[k][1], *origin(f), HS, WS) == 0)[:, :, None] for k, f in enumerate(flows)]
    assert sum(int(v.sum()) for v in visible_nan) > 5                       # NaN * 1 keeps its bits (compared above)
    assert all(b.min() == 0 and b.max() == 1 for _, b in inv + occ)
    # an example with an invalid row is skipped whole; a launch of one example writes map 1 right behind map 0's single slot
    one = torch.stack([table[3 * n], table[n], table[2 * n]])
    flow.fill_(CANARY)
    mask.fill_(CANARY)
    _lib.check(L.unflow_sintel_gt(_lib.ptr(raw_dev), _lib.cl(n_raw), _lib.ptr(dec), _lib.cl(dst), _lib.ptr(one), 1, HS, WS,
                                  _lib.ptr(flow), _lib.ptr(mask), _lib.stream(DEV)), "sintel_gt")
    assert (flow == CANARY).all() and (mask == CANARY).all()
    one[0] = table[0]
    _lib.check(L.unflow_sintel_gt(_lib.ptr(raw_dev), _lib.cl(n_raw), _lib.ptr(dec), _lib.cl(dst), _lib.ptr(one), 1, HS, WS,
                                  _lib.ptr(flow), _lib.ptr(mask), _lib.stream(DEV)), "sintel_gt")
    got = flow.cpu().numpy().reshape(2 * n, HS, WS, 2)
    assert F.same_bits(got[0], gf[0, 0]) and F.same_bits(got[1], gf[1, 0]) and (got[2:] == CANARY).all()


# ------------------------------------------------------------------------------------------------------------- loaders
DIMS = (16, 20)
SIZES = [(11, 13), (18, 24), (16, 20)]                 # below, above and equal to DIMS


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """Three examples per reader, frame sizes below, above and equal to DIMS, so B = 2 gives a full and a short batch."""
    root = tmp_path_factory.mktemp("flo_trees")
    scenes = [(2, s) for s in SIZES]
    F.make_sintel(root, scenes, seed=32, test_scenes=scenes)
    F.make_chairs(root, SIZES, seed=33, raw=(3, DIMS), unknown=0.1)
    F.make_middlebury(root, scenes, seed=34, unknown=0.1)
    return root


def assert_batches_equal(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, torch.Tensor):
            assert g.device == DEV and g.dtype == torch.float32, (what, j)
            assert F.same_bits(g.cpu().numpy(), w), "%s, array %d" % (what, j)
        else:
            assert j == 2 and g.dtype == np.int32 and np.array_equal(g, w), (what, j)          # input_shape stays on the host


READERS = {
    "sintel_train_clean": (SintelInput, "input_train_clean", 7),
    "sintel_test_final": (SintelInput, "input_test_final", 3),
    "chairs_test": (ChairsInput, "input_test", 5),
    "mdb_train": (MiddleburyInput, "input_train", 5),
}


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("reader", sorted(READERS))
def test_readers_on_the_device_equal_the_host(trees, reader, normalize):
    cls, name, width = READERS[reader]
    inp = cls(F.Data(trees), 2, DIMS, normalize=normalize)
    want = list(getattr(inp, name)())
    it = getattr(inp, name)(device=DEV, workers=4, prefetch=1)
    assert type(it) is D.DeviceEvalBatches
    got = [[t.clone() if isinstance(t, torch.Tensor) else t for t in batch] for batch in it]
    assert [b[0].shape[0] for b in got] == [2, 1] and len(want) == 2          # a short last batch
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == width
        assert_batches_equal(g, w, "%s batch %d" % (reader, k))
    assert not loader_threads()
    with pytest.raises(StopIteration):
        next(it)


@pytest.mark.parametrize("normalize", [False, True])
def test_chairs_input_raw_on_the_device_equals_the_host(trees, normalize, capsys):
    ch = ChairsInput(F.Data(trees, raw_dirs=['flying_chairs/image']), 2, DIMS, normalize=normalize)
    ref = ch.input_raw(swap_images=True, shift=1)
    it = ch.input_raw(swap_images=True, shift=1, device=DEV, workers=2, prefetch=1)
    assert type(it) is D.DevicePairBatches
    try:
        kept = [[t.clone() for t in next(it)] for _ in range(4)]           # six swapped pairs: the walk wraps
    finally:
        it.close()
    for k, got in enumerate(kept):
        want = next(ref)
        assert len(got) == 2 and all(F.same_bits(g.cpu().numpy(), w) for g, w in zip(got, want)), k
    assert not loader_threads()


def test_a_flo_file_that_changes_under_the_loader_is_an_error(tmp_path, monkeypatch):
    F.make_chairs(tmp_path, [(8, 10)] * 2, seed=35)
    ch = ChairsInput(F.Data(tmp_path), 1, (8, 10), normalize=False)
    flo = str(tmp_path / 'flying_chairs/flow/00002_flow.flo')
    with monkeypatch.context() as m:
        m.setattr(D, "flo_header", lambda p: (8, 10))   # the planner trusts the header it saw; the worker reads the file again
        I.write_flo(flo, np.zeros((8, 11, 2), np.float32))
        with pytest.raises(ValueError, match="00002_flow.flo changed on disk"):
            list(ch.input_test(device=DEV))
    assert not loader_threads()
    with open(flo, 'ab') as f:
        f.write(b'\0')
    with pytest.raises(ValueError, match="00002_flow.flo"):              # a file with trailing bytes: the planner refuses it by name
        list(ch.input_test(device=DEV))
    assert not loader_threads()


# ------------------------------------------------------------------------------------------------------------- consumers
def scaled_params(eng, seed):
    tfp = eng.init_params(seed=seed)
    return {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}


def files_of(folder):
    return {n: open(os.path.join(folder, n), 'rb').read() for n in sorted(os.listdir(folder))}


FRAMES = [(60, 120), (64, 128), (70, 133)]


@pytest.fixture(scope="module")
def estimator():
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(72, 136), device=DEV, bidirectional=True, visual=True)
    tfp = scaled_params(est.engine, 6)
    est.load_tf_params(tfp)
    return est, tfp


def compare_exports(est, batches, tmp_path, runs):
    for name, kw in runs:
        a = est.export(batches(None), str(tmp_path / (name + "_host")), **kw)
        b = est.export(batches(DEV), str(tmp_path / (name + "_dev")), **kw)
        assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b]
        fa, fb = files_of(str(tmp_path / (name + "_host"))), files_of(str(tmp_path / (name + "_dev")))
        assert list(fa) == list(fb) and len(fa) == len(a) > 0
        for n in fa:
            assert fa[n] == fb[n], n
    pics_h, pics_d = list(est.pictures(batches(None))), list(est.pictures(batches(DEV)))
    assert len(pics_d) == len(pics_h) == 3
    for ph, pd in zip(pics_h, pics_d):
        assert list(ph) == list(pd) and 'error' in pd and all(np.array_equal(ph[k], pd[k]) for k in ph)


def test_estimator_scores_sintel_from_device_batches_identically(tmp_path, estimator):
    est, _ = estimator
    F.make_sintel(tmp_path / "data", [(2, s) for s in FRAMES], seed=36)
    sin = SintelInput(F.Data(tmp_path / "data"), 2, (64, 128), normalize=False)
    batches = lambda dev: sin.input_train_clean(device=dev)        # noqa: E731
    want = est.evaluate(batches(None))
    got = est.evaluate(batches(DEV))
    assert want['names'] == ['AEE/occluded', 'outliers/occluded', 'AEE/non-occluded', 'outliers/non-occluded']
    assert want['num_examples'] == 3 and 'occ/F1' in want and len(want['occ_counts']) == 3
    assert all(np.isfinite(r).all() for r in want['per_example']) and sum(c[0] + c[2] for c in want['occ_counts']) > 0
    assert got == want                                              # every score, per-example row and occlusion count
    compare_exports(est, batches, tmp_path, (("all", dict(fmt='flo', backward=True, occlusion=True, visual=True)), ("two", dict(num=2))))
    assert not loader_threads()


def test_estimator_scores_one_map_chairs_with_unknown_pixels(tmp_path, estimator):
    est, _ = estimator
    flows = F.make_chairs(tmp_path / "data", FRAMES, seed=37, unknown=0.05, values=[1e10])
    assert all((f == np.float32(1e10)).any() for f in flows)
    ch = ChairsInput(F.Data(tmp_path / "data"), 2, (64, 128), normalize=False)
    batches = lambda dev: ch.input_test(device=dev)                # noqa: E731
    want = est.evaluate(batches(None))
    got = est.evaluate(batches(DEV))
    assert want['names'] == ['AEE/all', 'outliers/all'] and want['num_examples'] == 3 and 'occ/F1' not in want
    assert np.isfinite(want['per_example']).all() and np.isfinite([want['AEE/all'], want['outliers/all']]).all()
    assert 0 < want['AEE/all'] < 100                                # the 1e10 markers are masked out, not averaged in
    assert got == want
    compare_exports(est, batches, tmp_path, (("vis", dict(visual=True)),))
    assert not loader_threads()


def test_evaluate_flo_command_line(tmp_path, estimator, capsys):
    from unflow_amd import evaluate_flo as E
    from unflow_amd.core.input import save_checkpoint
    _, tfp = estimator
    F.make_sintel(tmp_path / "data", [(2, s) for s in [(60, 120), (64, 128), (59, 101)]], seed=38)
    ck = tmp_path / "ckpt" / "run"
    ck.mkdir(parents=True)
    save_checkpoint(str(ck / "model.ckpt-7"), tfp, 7)
    (ck / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-7"\n')
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\ndata = %s\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n"
                   % (tmp_path / "data", tmp_path / "log", tmp_path / "ckpt"))
    argv = ['--dataset', 'sintel', '--variant', 'train_final', '--ex', 'run', '--num', '-1', '--batch_size', '2', '--dims', '64', '128',
            '--config', str(cfg), '--occlusion', '--output_benchmark', '--output_backward', '--visual', '--sheet']
    assert E.main(argv + ['--out', str(tmp_path / "dev")]) == 0
    out = capsys.readouterr().out
    assert all(k in out for k in ('AEE/occluded', 'outliers/non-occluded', 'occ/F1', 'examples: 3'))
    assert E.main(argv + ['--out', str(tmp_path / "host"), '--host_decode']) == 0
    assert capsys.readouterr().out.replace(str(tmp_path / "host"), str(tmp_path / "dev")) == out
    fd, fh = files_of(str(tmp_path / "dev" / "run")), files_of(str(tmp_path / "host" / "run"))
    assert fd == fh
    for n in range(3):
        for name in ('%06d_10.flo', '%06d_01.flo', '%06d_10_occ.png', '%06d_img.png', '%06d_err.png', '%06d_gt.png'):
            assert name % n in fd
    assert 'page_000.png' in fd and 'config.ini' in fd
    assert not loader_threads()
