"""Mirror of src/e2eflow/sintel/input.py without TF queues: Sintel's clean / final passes, consecutive frames per scene folder,
with the two-map ground truth composed of each pair's .flo file and its `invalid` and `occlusions` PNGs (:86-105):

    flow_occ = flow                 mask_occ = 1 - invalid
    flow_noc = flow * (1 - occ)     mask_noc = mask_occ * (1 - occ)

after all three were cropped / zero-padded to the input's dims (so a padded pixel has flow 0 and both masks 1; evaluation crops
the padding away again).  invalid and occ are BINARY here — 1 where channel 0 of the PNG (a 16-bit sample's high byte) is
non-zero: the reference feeds the raw 0 / 255 grey values into 1 - invalid, which makes mask_occ = -254; the evident meaning of a
binary mask is followed.  The .flo size comes from the file's header, not the reference's hard-coded 436 x 1024.
Host numpy batches, or — with a device — the same batches as device tensors, composed by unflow_sintel_gt
(middlebury/input.py::FloInput, core/png_device.py).  input_train_gt (this project's addition) is the supervised
training input: random crops with one of the two composed maps.  The dataset downloader (sintel/data.py) is out of scope."""
import os

import numpy as np

from ..core.input import read_flo, read_png_image
from ..middlebury.input import FloInput, listed, scene_files, scene_pairs


def read_binary(path):
    """A mask PNG -> float32 [H,W,1] of 0 / 1: channel 0 (read_png_image's channel rule) != 0."""
    return (read_png_image(path)[:, :, :1] != 0).astype(np.float32)


class SintelInput(FloInput):
    def gt_files(self):
        """_input_flow's three listings (:86-94): flow, invalid without each scene's last file (invalid has a map per FRAME,
        flow and occlusions one per PAIR), occlusions.  Their lengths must agree."""
        flow = listed(self._dir('sintel/training/flow'))
        invalid = listed(self._dir('sintel/training/invalid'), drop_last=True)
        occ = listed(self._dir('sintel/training/occlusions'))
        if not len(flow) == len(invalid) == len(occ):
            raise ValueError("sintel: %d flow files, %d invalid maps (each scene's last dropped), %d occlusion maps"
                             % (len(flow), len(invalid), len(occ)))
        return [flow, invalid, occ]

    def train_files(self, image_dir):
        pairs, gt = scene_pairs(self._dir(image_dir)), self.gt_files()
        if len(pairs) != len(gt[0]):
            raise ValueError("sintel: %d frame pairs in %s but %d flow files" % (len(pairs), image_dir, len(gt[0])))
        return pairs, gt

    def clips(self, variant='clean'):
        """The scenes of sintel/training/<variant> as clips: a list of (scene name, frame files, [(flo, invalid,
        occlusions), ...]), the triple of pair i = (frame i, frame i + 1) at position i — gt_files' three listings scene by
        scene, with its length checks per scene: a scene of T frames has T - 1 flow files, T invalid maps (the last dropped) and
        T - 1 occlusion maps."""
        if variant not in ('clean', 'final'):
            raise ValueError("variant must be 'clean' or 'final', got %r" % (variant,))
        image_dir = 'sintel/training/' + variant
        self.train_files(image_dir)                  # the listings' total lengths agree
        names = sorted(os.listdir(self._dir(image_dir)))
        frames = scene_files(self._dir(image_dir))
        flow = scene_files(self._dir('sintel/training/flow'))
        invalid = scene_files(self._dir('sintel/training/invalid'), drop_last=True)
        occ = scene_files(self._dir('sintel/training/occlusions'))
        if not len(frames) == len(flow) == len(invalid) == len(occ):
            raise ValueError("sintel: %d scenes in %s, %d in flow, %d in invalid, %d in occlusions"
                             % (len(frames), image_dir, len(flow), len(invalid), len(occ)))
        out = []
        for name, fr, fl, inv, oc in zip(names, frames, flow, invalid, occ):
            if not len(fr) - 1 == len(fl) == len(inv) == len(oc):
                raise ValueError("sintel: scene %s has %d frames (%d pairs) but %d flow files, %d invalid maps (its last dropped), "
                                 "%d occlusion maps" % (name, len(fr), max(len(fr) - 1, 0), len(fl), len(inv), len(oc)))
            out.append((name, fr, list(zip(fl, inv, oc))))
        return out

    def read_gt_full(self, f_flow, f_invalid, f_occ):
        """_read_gt's composition at the files' own size, no crop and no padding: (flow_occ [h,w,2], mask_occ [h,w], flow_noc,
        mask_noc) — what evaluate_flo --sequence scores a clip against (png_device.sintel_gt_device: the same bits)."""
        flow = read_flo(f_flow)[0].numpy()
        invalid, occ = read_binary(f_invalid), read_binary(f_occ)
        for f, m in ((f_invalid, invalid), (f_occ, occ)):
            if m.shape[:2] != flow.shape[:2]:
                raise ValueError("%s is %d x %d, its flow file %s %d x %d" % ((f,) + m.shape[:2] + (f_flow,) + flow.shape[:2]))
        mask_occ = 1 - invalid
        return flow, mask_occ[:, :, 0], flow * (1 - occ), (mask_occ * (1 - occ))[:, :, 0]

    def _read_gt(self, f_flow, f_invalid, f_occ):
        flow = read_flo(f_flow)[0].numpy()
        invalid, occ = read_binary(f_invalid), read_binary(f_occ)
        for f, m in ((f_invalid, invalid), (f_occ, occ)):
            if m.shape[:2] != flow.shape[:2]:
                raise ValueError("%s is %d x %d, its flow file %s %d x %d" % ((f,) + m.shape[:2] + (f_flow,) + flow.shape[:2]))
        flow, invalid, occ = self._preprocess_map(flow), self._preprocess_map(invalid), self._preprocess_map(occ)
        mask_occ = 1 - invalid
        return flow, mask_occ, flow * (1 - occ), mask_occ * (1 - occ)

    def _window_gt(self, files, oy, ox):
        """_read_gt's composition on the (dims) window at (oy, ox) instead of the central crop / padding: (flow_occ, mask_occ,
        flow_noc, mask_noc).  The window must lie inside all three maps (ValueError naming the file)."""
        from ..core.png_device import check_window_inside
        f_flow, f_invalid, f_occ = files
        h, w = self.dims
        flow = read_flo(f_flow)[0].numpy()
        invalid, occ = read_binary(f_invalid), read_binary(f_occ)
        check_window_inside(f_flow, flow.shape, oy, ox, self.dims)
        for f, m in ((f_invalid, invalid), (f_occ, occ)):
            if m.shape[:2] != flow.shape[:2]:
                raise ValueError("%s is %d x %d, its flow file %s %d x %d" % ((f,) + m.shape[:2] + (f_flow,) + flow.shape[:2]))
        flow, invalid, occ = (a[oy:oy + h, ox:ox + w] for a in (flow, invalid, occ))
        mask_occ = 1 - invalid
        return flow, mask_occ, flow * (1 - occ), mask_occ * (1 - occ)

    def input_train_gt(self, variant='clean', gt='occ', seed=0, shift=0, device=None, workers=8, prefetch=2):
        """The supervised training input (this project's addition; the reference has none for Sintel): an endless iterator of
        (im1, im2, flow_gt, mask_gt) over the pairs of sintel/training/<variant> with the composed ground truth of _read_gt —
        gt 'occ': (flow, 1 - invalid), 'noc': (flow * (1 - occ), (1 - invalid) * (1 - occ)) — one random window of self.dims
        per example, as KITTIInput.input_train_gt draws it (FloInput._train_gt_host).  device: the same batches, bit for
        bit, as device tensors (core/png_device.py::DeviceGTBatches, composed by unflow_sintel_gt)."""
        if variant not in ('clean', 'final'):
            raise ValueError("variant must be 'clean' or 'final', got %r" % (variant,))
        if gt not in ('occ', 'noc'):
            raise ValueError("gt must be 'occ' or 'noc', got %r" % (gt,))
        pairs, lists = self.train_files('sintel/training/' + variant)
        examples = [tuple(p) + tuple(g[k] for g in lists) for k, p in enumerate(pairs)]
        return self._train_gt(examples, 'sintel', ('occ', 'noc').index(gt), seed, shift, device, workers, prefetch)

    def _input_train(self, image_dir, device, workers, prefetch):
        """_input_train (:107-114): batches of (im1, im2, input_shape, flow_occ, mask_occ, flow_noc, mask_noc)."""
        return self._batches(lambda: self.train_files(image_dir), 'sintel', device, workers, prefetch)

    def _input_test(self, image_dir, device, workers, prefetch):
        return self._batches(lambda: (scene_pairs(self._dir(image_dir)), []), None, device, workers, prefetch)

    def input_train_clean(self, device=None, workers=8, prefetch=2):
        return self._input_train('sintel/training/clean', device, workers, prefetch)

    def input_train_final(self, device=None, workers=8, prefetch=2):
        return self._input_train('sintel/training/final', device, workers, prefetch)

    def input_test_clean(self, device=None, workers=8, prefetch=2):
        """input_test_clean (:122-128): batches of (im1, im2, input_shape)."""
        return self._input_test('sintel/test/clean', device, workers, prefetch)

    def input_test_final(self, device=None, workers=8, prefetch=2):
        return self._input_test('sintel/test/final', device, workers, prefetch)
