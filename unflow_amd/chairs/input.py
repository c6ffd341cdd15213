"""Mirror of src/e2eflow/chairs/input.py without TF queues: FlyingChairs' test pairs with their .flo ground truth (one map), and
the raw training pairs — and, this project's addition, the supervised training input input_train_gt (random crops of the
training pairs with the .flo files of flying_chairs/train_flow).  Host numpy batches, or — with a device — the same batches as device tensors (middlebury/input.py::
FloInput).  The dataset downloader and its .ppm conversion (chairs/data.py) are out of scope: the frames are PNG files."""
import os

from ..middlebury.input import FloInput


class ChairsInput(FloInput):
    def test_files(self):
        """(Input.test_pairs('flying_chairs/test_image'): files 2i and 2i + 1 of the sorted listing, [the sorted
        flying_chairs/flow]), paired position by position as the reference's queues do; differing counts raise."""
        pairs = self.test_pairs('flying_chairs/test_image')
        flow_dir = self._dir('flying_chairs/flow')
        flows = [os.path.join(flow_dir, fn) for fn in sorted(os.listdir(flow_dir))]
        if len(pairs) != len(flows):
            raise ValueError("flying_chairs: %d frame pairs in test_image but %d flow files in flow" % (len(pairs), len(flows)))
        return pairs, [flows]

    def input_test(self, device=None, workers=8, prefetch=2):
        """input_test (:30-37): batches of (im1, im2, input_shape, flow, mask)."""
        return self._batches(self.test_files, 'flo', device, workers, prefetch)

    def train_gt_files(self, flow_dir='flying_chairs/train_flow'):
        """[(im1, im2, .flo)]: files 2i and 2i + 1 of the sorted flying_chairs/image with file i of the sorted `flow_dir`,
        position by position; differing counts raise.  `flow_dir` is THIS PROJECT's addition to the data layout: the
        reference's converter (chairs/data.py) throws the training flows away, so the directory has to be filled with the
        dataset's %05d_flow.flo files of the training split."""
        pairs = self.test_pairs('flying_chairs/image')
        d = self._dir(flow_dir)
        flows = [os.path.join(d, fn) for fn in sorted(os.listdir(d))]
        if len(pairs) != len(flows):
            raise ValueError("flying_chairs: %d frame pairs in image but %d flow files in %s" % (len(pairs), len(flows), flow_dir))
        return [(a, b, f) for (a, b), f in zip(pairs, flows)]

    def input_train_gt(self, flow_dir='flying_chairs/train_flow', seed=0, shift=0, device=None, workers=8, prefetch=2):
        """The supervised training input (this project's addition): an endless iterator of (im1, im2, flow_gt, mask_gt) over
        train_gt_files(flow_dir), mask = (u < 1e9 and v < 1e9), one random window of self.dims per example as
        KITTIInput.input_train_gt draws it (FloInput._train_gt_host).  device: the same batches, bit for bit, as device
        tensors (core/png_device.py::DeviceGTBatches, unflow_flo_to_flow_gt)."""
        return self._train_gt(self.train_gt_files(flow_dir), 'flo', 0, seed, shift, device, workers, prefetch)

    def input_raw(self, swap_images=True, shift=0, device=None, workers=8, prefetch=2):
        """input_raw (:39-43): uncorrelated pairs (files 2i, 2i + 1 of each raw directory), frames of exactly self.dims."""
        return super().input_raw(swap_images=swap_images, shift=shift, sequence=False, needs_crop=False, device=device,
                                 workers=workers, prefetch=prefetch)
