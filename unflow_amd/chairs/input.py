"""Mirror of src/e2eflow/chairs/input.py without TF queues: FlyingChairs' test pairs with their .flo ground truth (one map), and
the raw training pairs.  Host numpy batches, or — with a device — the same batches as device tensors (middlebury/input.py::
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

    def input_raw(self, swap_images=True, shift=0, device=None, workers=8, prefetch=2):
        """input_raw (:39-43): uncorrelated pairs (files 2i, 2i + 1 of each raw directory), frames of exactly self.dims."""
        return super().input_raw(swap_images=swap_images, shift=shift, sequence=False, needs_crop=False, device=device,
                                 workers=workers, prefetch=prefetch)
