"""Mirror of src/e2eflow/kitti/input.py without TF queues: the evaluation inputs of Trainer.eval (train.py:265-385) — image
pairs of a KITTI `training` directory with their occluded / non-occluded ground-truth flow maps, batch 1, one epoch — and the
supervised fine-tuning input input_train_gt (:86-146): KITTI 2015 + 2012 pairs with their flow_occ maps, jointly cropped.
The dataset downloaders (kitti/data.py) are out of scope."""
import os
import random

import numpy as np

from ..core.input import Input, decode_png, read_kitti_flow_png, read_png_image, resize_image_with_crop_or_pad


class KITTIInput(Input):
    def __init__(self, data, batch_size, dims, *, num_threads=1, normalize=True, skipped_frames=False):
        super().__init__(data, batch_size, dims, num_threads=num_threads, normalize=normalize, skipped_frames=skipped_frames)

    def _preprocess_flow(self, gt):
        """kitti/input.py:32-38: flow and validity mask cropped / zero-padded to the input's dims."""
        flow, mask = gt
        h, w = self.dims
        return (resize_image_with_crop_or_pad(flow.numpy(), h, w).reshape(h, w, 2),
                resize_image_with_crop_or_pad(mask.numpy(), h, w).reshape(h, w, 1))

    def _flow_files(self, flow_dir, hold_out_inv):
        """kitti/input.py:40-66: the sorted listings of flow_occ / flow_noc, each cut to the first hold_out_inv entries of
        its own seed-0 shuffle."""
        out = []
        for sub in ('flow_occ', 'flow_noc'):
            d = os.path.join(self.data.current_dir, flow_dir, sub)
            files = sorted(os.listdir(d))
            if hold_out_inv is not None:
                random.seed(0)
                random.shuffle(files)
                files = files[:hold_out_inv]
            out.append([os.path.join(d, f) for f in files])
        assert len(out[0]) == len(out[1])
        return out

    def _input_train(self, image_dir, flow_dir, hold_out_inv=None, device=None, workers=8, prefetch=2):
        """kitti/input.py:75-82: batches of [im1, im2, input_shape, flow_occ, mask_occ, flow_noc, mask_noc] (numpy,
        NHWC), one epoch, a smaller final batch allowed.  The images come from Input.input_test's pair list (same
        hold-out shuffle), the ground truth from _flow_files, position by position as the reference's queues pair them.
        device: None = decoded on the host; a GPU device = the same batches, bit for bit, as device tensors (input_shape stays a
        host array) from the library's PNG kernels (core/png_device.py::DeviceEvalBatches)."""
        if device is not None:
            from ..core.png_device import DeviceEvalBatches
            pairs, occ, noc = self._eval_files(image_dir, flow_dir, hold_out_inv)
            return DeviceEvalBatches(pairs, self.batch_size, self.dims, self.normalize, self.mean, self.stddev, gt_lists=(occ, noc),
                                     device=device, workers=workers, prefetch=prefetch)
        return self._input_train_host(image_dir, flow_dir, hold_out_inv)

    def _eval_files(self, image_dir, flow_dir, hold_out_inv):
        pairs = self.test_pairs(image_dir, hold_out_inv)
        occ, noc = self._flow_files(flow_dir, hold_out_inv)
        assert len(pairs) == len(occ), (len(pairs), len(occ))
        return pairs, occ, noc

    def _input_train_host(self, image_dir, flow_dir, hold_out_inv):
        pairs, occ, noc = self._eval_files(image_dir, flow_dir, hold_out_inv)    # a generator: listed at the first next(), as ever
        for b0 in range(0, len(pairs), self.batch_size):
            cols = [[] for _ in range(7)]
            for (fn1, fn2), f_occ, f_noc in zip(pairs[b0:b0 + self.batch_size], occ[b0:], noc[b0:]):
                a, b = read_png_image(fn1), read_png_image(fn2)
                fo, mo = self._preprocess_flow(read_kitti_flow_png(f_occ))
                fnc, mn = self._preprocess_flow(read_kitti_flow_png(f_noc))
                for c, v in zip(cols, (self._preprocess_image(a), self._preprocess_image(b), np.asarray(a.shape, dtype=np.int32),
                                       fo, mo, fnc, mn)):
                    c.append(v)
            yield tuple(np.stack(c) for c in cols)

    def input_train_2015(self, hold_out_inv=None, device=None, workers=8, prefetch=2):
        return self._input_train('data_scene_flow/training/image_2', 'data_scene_flow/training', hold_out_inv, device, workers,
                                 prefetch)

    def input_test_2015(self, hold_out_inv=None, device=None, workers=8, prefetch=2):
        return self.input_test('data_scene_flow/testing/image_2', hold_out_inv, device, workers, prefetch)

    def input_train_2012(self, hold_out_inv=None, device=None, workers=8, prefetch=2):
        return self._input_train('data_stereo_flow/training/colored_0', 'data_stereo_flow/training', hold_out_inv, device, workers,
                                 prefetch)

    def input_test_2012(self, hold_out_inv=None, device=None, workers=8, prefetch=2):
        return self.input_test('data_stereo_flow/testing/colored_0', hold_out_inv, device, workers, prefetch)

    def train_gt_files(self, hold_out):
        """The example list of input_train_gt (kitti/input.py:86-124): per dataset (2015 image_2 + flow_occ, 2012 colored_0 +
        flow_occ) images 2i and 2i+1 of the sorted listing go with GT file i; each list is shuffled with seed 0 and its first
        `hold_out` entries dropped; the concatenation is shuffled again with seed 0.  [(im1, im2, gt), ...]."""
        img_dirs = ['data_scene_flow/training/image_2', 'data_stereo_flow/training/colored_0']
        gt_dirs = ['data_scene_flow/training/flow_occ', 'data_stereo_flow/training/flow_occ']
        filenames = []
        for img_dir, gt_dir in zip(img_dirs, gt_dirs):
            img_dir = os.path.join(self.data.current_dir, img_dir)
            gt_dir = os.path.join(self.data.current_dir, gt_dir)
            img_files, gt_files = sorted(os.listdir(img_dir)), sorted(os.listdir(gt_dir))
            assert len(img_files) % 2 == 0 and len(img_files) / 2 == len(gt_files)
            ds = [(os.path.join(img_dir, img_files[2 * i]), os.path.join(img_dir, img_files[2 * i + 1]),
                   os.path.join(gt_dir, gt_files[i])) for i in range(len(gt_files))]
            random.seed(0)
            random.shuffle(ds)
            filenames.extend(ds[hold_out:])
        random.seed(0)
        random.shuffle(filenames)
        return filenames

    def input_train_gt(self, hold_out, seed=0, shift=0, device=None, workers=8, prefetch=2):
        """The supervised fine-tuning input: _input_train_gt_host's batches, decoded on the host (device None) or — the same
        batches, bit for bit, as device tensors — by the library's PNG kernels with `workers` inflate threads and `prefetch`
        batches in flight (core/png_device.py::DeviceGTBatches)."""
        if device is not None:
            from ..core.png_device import DeviceGTBatches
            return DeviceGTBatches(self.train_gt_files(hold_out), self.batch_size, self.dims, self.normalize, self.mean,
                                   self.stddev, seed=seed, shift=shift, device=device, workers=workers, prefetch=prefetch)
        return self._input_train_gt_host(hold_out, seed, shift)

    def _input_train_gt_host(self, hold_out, seed=0, shift=0):
        """input_train_gt (kitti/input.py:86-146): an endless iterator of (im1, im2, flow_gt, mask_gt) numpy batches
        [B,h,w,3] x 2, [B,h,w,2], [B,h,w,1] over train_gt_files(hold_out), walked in order and cyclically like the
        reference's string_input_producer(shuffle=False); random_crop takes ONE window of self.dims for both frames and the
        16-bit GT (limit from im1's shape, RNG seeded with `seed`), the GT decodes as flow = (v - 2^15) / 64, mask = channel
        2; the images are normalised when self.normalize.  shift: examples to skip at the start (resuming)."""
        files = self.train_gt_files(hold_out)
        h, w = self.dims
        rng = np.random.RandomState(seed)
        pos = shift
        while True:
            cols = [[] for _ in range(4)]
            for _ in range(self.batch_size):
                fn1, fn2, fgt = files[pos % len(files)]
                pos += 1
                a, b = read_png_image(fn1), read_png_image(fn2)
                with open(fgt, 'rb') as f:
                    gt = decode_png(f.read()).astype(np.float32)
                oy = int(rng.randint(0, a.shape[0] - h + 1))
                ox = int(rng.randint(0, a.shape[1] - w + 1))
                a, b, gt = a[oy:oy + h, ox:ox + w], b[oy:oy + h, ox:ox + w], gt[oy:oy + h, ox:ox + w]
                flow = (gt[:, :, 0:2] - 2 ** 15) / 64.0
                mask = gt[:, :, 2:3]
                if self.normalize:
                    a, b = self._normalize_image(a), self._normalize_image(b)
                for c, v in zip(cols, (a, b, flow, mask)):
                    c.append(v)
            yield tuple(np.stack(c).astype(np.float32) for c in cols)
