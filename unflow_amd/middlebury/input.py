"""Mirror of src/e2eflow/middlebury/input.py without TF queues: the Middlebury evaluation inputs, and what the three .flo
datasets (Middlebury, FlyingChairs, Sintel) share — the per-scene listings and FloInput, the reader of frame pairs with or
without ground truth.  With device=None a reader is a host generator of numpy batches (one epoch, a smaller final batch
allowed); with a GPU device it yields the same batches, bit for bit, as device tensors from core/png_device.py::DeviceEvalBatches
(input_shape stays a host array).  The dataset downloaders (middlebury/data.py) are out of scope."""
import os

import numpy as np

from ..core.input import Input, read_flo, read_png_image, resize_image_with_crop_or_pad


def scene_files(root, drop_last=False):
    """The listing all three datasets' per-scene folders share (_get_filenames, :41-52; _input_images, :66-81): one list of full
    paths per scene, the scenes and each scene's files in sorted order.  drop_last: without each scene's last file (Sintel's
    `invalid` holds a map per frame where `flow` and `occlusions` hold one per pair)."""
    scenes = []
    for scene in sorted(os.listdir(root)):
        files = [os.path.join(root, scene, name) for name in sorted(os.listdir(os.path.join(root, scene)))]
        scenes.append(files[:-1] if drop_last else files)
    return scenes


def listed(root, drop_last=False):
    """scene_files as one list: the order in which ground-truth files pair up with scene_pairs."""
    return [f for files in scene_files(root, drop_last) for f in files]


def scene_pairs(root):
    """Every consecutive pair (file i, file i + 1) of each scene, scene by scene (_input_images, :66-81)."""
    return [pair for files in scene_files(root) for pair in zip(files[:-1], files[1:])]


class FloInput(Input):
    """Input plus the evaluation readers of the .flo datasets.  A subclass names its files: `files` is a callable that returns
    (pairs, ground-truth lists), called at the first next() of a host generator (as Input's readers list their directories) and
    at once for a device reader."""

    def _dir(self, sub):
        return os.path.join(self.data.current_dir, sub)

    def _preprocess_map(self, a):
        """_preprocess_flow (:61-64): a ground-truth map cropped / zero-padded to the input's dims."""
        h, w = self.dims
        return resize_image_with_crop_or_pad(a, h, w).reshape(h, w, a.shape[2])

    def _read_gt(self, *files):
        """One example's ground truth, preprocessed: (flow [h,w,2], mask [h,w,1]) of a .flo file (_read_flow, :10-28)."""
        flow, mask = read_flo(files[0])
        return self._preprocess_map(flow.numpy()), self._preprocess_map(mask.numpy())

    def _batches(self, files, gt_kind, device, workers, prefetch):
        if device is not None:
            from ..core.png_device import DeviceEvalBatches
            pairs, gt_lists = files()
            return DeviceEvalBatches(pairs, self.batch_size, self.dims, self.normalize, self.mean, self.stddev, gt_lists=gt_lists,
                                     gt_kind=gt_kind, device=device, workers=workers, prefetch=prefetch)
        return self._batches_host(files)

    def _batches_host(self, files):
        pairs, gt_lists = files()
        for b0 in range(0, len(pairs), self.batch_size):
            cols = None
            for k in range(b0, min(b0 + self.batch_size, len(pairs))):
                a, b = read_png_image(pairs[k][0]), read_png_image(pairs[k][1])
                row = (self._preprocess_image(a).astype(np.float32), self._preprocess_image(b).astype(np.float32),
                       np.asarray(a.shape, dtype=np.int32))
                if gt_lists:
                    row += tuple(self._read_gt(*[g[k] for g in gt_lists]))
                cols = cols or [[] for _ in row]
                for c, v in zip(cols, row):
                    c.append(v)
            yield tuple(np.stack(c) for c in cols)


    # ---- supervised training input (this project's addition): the twin of KITTIInput.input_train_gt
    def _window_gt(self, files, oy, ox):
        """One example's ground truth on the (dims) window at (oy, ox): (flow [h,w,2], mask [h,w,1]) of a .flo file."""
        from ..core.png_device import check_window_inside
        h, w = self.dims
        flow, mask = read_flo(files[0])
        check_window_inside(files[0], flow.shape, oy, ox, self.dims)
        return flow.numpy()[oy:oy + h, ox:ox + w], mask.numpy()[oy:oy + h, ox:ox + w]

    def _train_gt(self, examples, gt_kind, gt_map, seed, shift, device, workers, prefetch):
        """examples: [(im1, im2, ground-truth files ...)].  Host generator, or the same batches from DeviceGTBatches."""
        if device is not None:
            from ..core.png_device import DeviceGTBatches
            return DeviceGTBatches(examples, self.batch_size, self.dims, self.normalize, self.mean, self.stddev, seed=seed,
                                   shift=shift, device=device, workers=workers, prefetch=prefetch, gt_kind=gt_kind, gt_map=gt_map)
        return self._train_gt_host(examples, gt_map, seed, shift)

    def _train_gt_host(self, examples, gt_map, seed, shift):
        """An endless iterator of (im1, im2, flow_gt, mask_gt) numpy batches [B,h,w,3] x 2, [B,h,w,2], [B,h,w,1]: the examples
        in order and cyclically from `shift`, per example ONE random window of self.dims for both frames and the ground truth
        — oy, then ox, from np.random.RandomState(seed), limits from im1 (KITTIInput._input_train_gt_host's draws).  A window
        that leaves one of the example's files raises ValueError naming it."""
        from ..core.png_device import check_window_inside
        h, w = self.dims
        rng = np.random.RandomState(seed)
        pos = shift
        while True:
            cols = [[] for _ in range(4)]
            for _ in range(self.batch_size):
                ex = examples[pos % len(examples)]
                pos += 1
                a, b = read_png_image(ex[0]), read_png_image(ex[1])
                check_window_inside(ex[0], a.shape, 0, 0, self.dims)
                oy = int(rng.randint(0, a.shape[0] - h + 1))
                ox = int(rng.randint(0, a.shape[1] - w + 1))
                check_window_inside(ex[1], b.shape, oy, ox, self.dims)
                flow, mask = self._window_gt(ex[2:], oy, ox)[2 * gt_map:2 * gt_map + 2]
                a, b = a[oy:oy + h, ox:ox + w], b[oy:oy + h, ox:ox + w]
                if self.normalize:
                    a, b = self._normalize_image(a), self._normalize_image(b)
                for c, v in zip(cols, (a, b, flow, mask)):
                    c.append(v)
            yield tuple(np.stack(c).astype(np.float32) for c in cols)


class MiddleburyInput(FloInput):
    def train_files(self):
        """(pairs of middlebury/other-data, [the .flo files of middlebury/other-gt-flow]).  The reference zips the two position
        by position and misaligns silently when a scene has more than two frames; differing counts raise here."""
        pairs = scene_pairs(self._dir('middlebury/other-data'))
        flows = listed(self._dir('middlebury/other-gt-flow'))
        if len(pairs) != len(flows):
            raise ValueError("middlebury: %d frame pairs in other-data but %d flow files in other-gt-flow" % (len(pairs), len(flows)))
        return pairs, [flows]

    def input_train(self, device=None, workers=8, prefetch=2):
        """input_train (:98-108): batches of (im1, im2, input_shape, flow, mask)."""
        return self._batches(self.train_files, 'flo', device, workers, prefetch)

    def input_test(self, device=None, workers=8, prefetch=2):
        """input_test (:110-116): batches of (im1, im2, input_shape) of middlebury/eval-data."""
        return self._batches(lambda: (scene_pairs(self._dir('middlebury/eval-data')), []), None, device, workers, prefetch)
