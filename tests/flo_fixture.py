"""Synthetic Sintel / FlyingChairs / Middlebury trees for the .flo input tests, written with the package's own encoders
(core/input.py: encode_png8_rgb, encode_png8_gray, write_flo) — filter-0 PNG files, so the host decoder reads them quickly — and
the bit-view comparison those tests share."""
import os

import numpy as np

from unflow_amd.core import input as I

SPECIAL = np.asarray([1e10, 1e9, np.nextafter(np.float32(1e9), np.float32(0)), np.inf, -np.inf, np.nan, -0.0, 0.0], dtype=np.float32)


class Data:
    def __init__(self, root, raw_dirs=()):
        self.current_dir = str(root)
        self._raw = [os.path.join(str(root), d) for d in raw_dirs]

    def get_raw_dirs(self):
        return self._raw


def bits(a):
    """The int32 bit view of a float32 array: -0 differs from +0, a NaN equals the NaN of the same payload."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def flow_field(rs, h, w, special=0.0, values=SPECIAL):
    """float32 [h, w, 2] within +-8 px; `special`: the fraction of components drawn from `values` (default SPECIAL: the 1e10
    marker, exactly 1e9, just below, infinities, NaN, -0)."""
    f = ((rs.rand(h, w, 2) - 0.5) * 16).astype(np.float32)
    if special:
        pick = rs.rand(h, w, 2) < special
        f[pick] = np.asarray(values, dtype=np.float32)[rs.randint(0, len(values), size=int(pick.sum()))]
    return f


def mask_map(rs, h, w, p=0.3):
    """uint8 [h, w] of 0, 1 and 255: non-zero with probability p."""
    return (np.asarray([1, 255], dtype=np.uint8)[rs.randint(0, 2, size=(h, w))] * (rs.rand(h, w) < p)).astype(np.uint8)


def _put(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)


def write_frame(path, rs, h, w):
    _put(path, I.encode_png8_rgb(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)))


def write_flo(path, flow):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    I.write_flo(path, flow)


def make_sintel(root, scenes, seed, test_scenes=(), unknown=0.0):
    """sintel/training/{clean,final,flow,invalid,occlusions}/<scene>/: scenes = [(frames, (h, w)), ...] — per scene `frames`
    frames in both passes, frames - 1 flow files and occlusion maps, `frames` invalid maps (the last one is never read: it is
    written with every pixel invalid).  The flow is negative under every occluded pixel of the first pair of a scene.
    test_scenes: the same for sintel/test/{clean,final}.  Returns {(scene index, pair index): (flow, invalid, occ)}."""
    rs = np.random.RandomState(seed)
    truth = {}
    tr = os.path.join(str(root), 'sintel', 'training')
    for s, (n, (h, w)) in enumerate(scenes):
        name = 'scene_%d' % s
        for i in range(n):
            for p in ('clean', 'final'):
                write_frame(os.path.join(tr, p, name, 'frame_%04d.png' % (i + 1)), rs, h, w)
            inv = mask_map(rs, h, w, 0.2) if i < n - 1 else np.full((h, w), 255, np.uint8)
            _put(os.path.join(tr, 'invalid', name, 'frame_%04d.png' % (i + 1)), I.encode_png8_gray(inv))
            if i == n - 1:
                continue
            flow, occ = flow_field(rs, h, w, unknown), mask_map(rs, h, w, 0.3)
            if i == 0:
                flow[occ != 0] = -np.abs(flow[occ != 0]) - np.float32(0.5)
            write_flo(os.path.join(tr, 'flow', name, 'frame_%04d.flo' % (i + 1)), flow)
            _put(os.path.join(tr, 'occlusions', name, 'frame_%04d.png' % (i + 1)), I.encode_png8_gray(occ))
            truth[(s, i)] = (flow, inv, occ)
    for s, (n, (h, w)) in enumerate(test_scenes):
        for i in range(n):
            for p in ('clean', 'final'):
                write_frame(os.path.join(str(root), 'sintel', 'test', p, 'test_%d' % s, 'frame_%04d.png' % (i + 1)), rs, h, w)
    return truth


def make_chairs(root, sizes, seed, raw=None, unknown=0.0, values=SPECIAL):
    """flying_chairs/test_image/%05d_img{1,2}.png and flying_chairs/flow/%05d_flow.flo, one example per entry of sizes; raw =
    (pairs, (h, w)): flying_chairs/image with that many uncorrelated pairs of exactly that size.  Returns the flows."""
    rs = np.random.RandomState(seed)
    base = os.path.join(str(root), 'flying_chairs')
    flows = []
    for i, (h, w) in enumerate(sizes):
        for k in (1, 2):
            write_frame(os.path.join(base, 'test_image', '%05d_img%d.png' % (i + 1, k)), rs, h, w)
        flows.append(flow_field(rs, h, w, unknown, values))
        write_flo(os.path.join(base, 'flow', '%05d_flow.flo' % (i + 1)), flows[-1])
    if raw:
        for i in range(raw[0]):
            for k in (1, 2):
                write_frame(os.path.join(base, 'image', '%05d_img%d.png' % (i + 1, k)), rs, *raw[1])
    return flows


def make_middlebury(root, scenes, seed, eval_scenes=(), unknown=0.05):
    """middlebury/other-data/<scene>/frame1{0,1,...}.png and other-gt-flow/<scene>/flow1{0,...}.flo: scenes = [(frames, (h, w)),
    ...], frames - 1 flow files per scene, the flow with a fraction `unknown` of special values (the 1e10 marker among them);
    eval_scenes: the same frames under eval-data.  Returns the flows in listing order."""
    rs = np.random.RandomState(seed)
    base = os.path.join(str(root), 'middlebury')
    flows = []
    for s, (n, (h, w)) in enumerate(scenes):
        for i in range(n):
            write_frame(os.path.join(base, 'other-data', 'scene_%d' % s, 'frame%d.png' % (10 + i)), rs, h, w)
        for i in range(n - 1):
            flows.append(flow_field(rs, h, w, unknown))
            write_flo(os.path.join(base, 'other-gt-flow', 'scene_%d' % s, 'flow%d.flo' % (10 + i)), flows[-1])
    for s, (n, (h, w)) in enumerate(eval_scenes):
        for i in range(n):
            write_frame(os.path.join(base, 'eval-data', 'eval_%d' % s, 'frame%d.png' % (10 + i)), rs, h, w)
    return flows
