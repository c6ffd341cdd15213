"""A synthetic KITTI tree with both supervised-training layouts (test infrastructure): data_scene_flow/training/{image_2,
flow_occ} (2015) and data_stereo_flow/training/{colored_0, flow_occ} (2012), frames 2i / 2i+1 with GT file i, written with
the package's own PNG encoders (u16 = 2^15 + 64 * flow, third channel = validity, kitti/input.py:12-22)."""
import os

import numpy as np

LAYOUTS = [('data_scene_flow/training/image_2', 'data_scene_flow/training/flow_occ'),
           ('data_stereo_flow/training/colored_0', 'data_stereo_flow/training/flow_occ')]


class Data:
    def __init__(self, root):
        self.current_dir = str(root)


def make_gt_tree(root, n_per_dataset=(3, 3), size=(72, 100), seed=0):
    """Returns {gt path: (im1, im2, flow, mask)} as written (float32; flow exact after the u16 quantisation)."""
    from unflow_amd.core import input as I
    rs = np.random.RandomState(seed)
    h, w = size
    out = {}
    for (img_dir, gt_dir), n in zip(LAYOUTS, n_per_dataset):
        di, dg = os.path.join(str(root), img_dir), os.path.join(str(root), gt_dir)
        os.makedirs(di, exist_ok=True)
        os.makedirs(dg, exist_ok=True)
        for i in range(n):
            im1 = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
            im2 = np.roll(im1, shift=(1, -2), axis=(0, 1))
            flow = np.round(rs.randn(h, w, 2) * 4.0 * 64.0) / 64.0
            valid = rs.rand(h, w) < 0.6
            u16 = np.zeros((h, w, 3), np.uint16)
            u16[..., :2] = (flow * 64.0 + 2 ** 15).astype(np.uint16)
            u16[..., 2] = valid
            fgt = os.path.join(dg, '%06d_10.png' % i)
            with open(fgt, 'wb') as f:
                f.write(I.encode_png16_rgb(u16))
            for k, im in ((10, im1), (11, im2)):
                with open(os.path.join(di, '%06d_%d.png' % (i, k)), 'wb') as f:
                    f.write(I.encode_png8_rgb(im))
            out[fgt] = (im1.astype(np.float32), im2.astype(np.float32), flow.astype(np.float32),
                        valid[..., None].astype(np.float32))
    return out
