"""Mirror of src/e2eflow/core/flow_util.py: the metrics (:98-123) and the visualisers flow_to_color / flow_error_image (:5-95),
the latter as HIP kernels (csrc/visual.hip) on device tensors."""
import ctypes

import torch

from .. import _lib
from .engine import flow_error_avg  # noqa: F401  (EPE, flow_util.py:98-103)


def _dense(t, c, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: a device tensor is required (the visualisers are HIP kernels)" % what)
    if t.dim() != 4 or t.shape[3] != c:
        raise ValueError("%s: expected [B,H,W,%d], got %s" % (what, c, tuple(t.shape)))
    return t.float().contiguous()


def flow_to_color(flow, mask=None, max_flow=None, uint8=False):
    """flow_util.py:20-43: flow [B,H,W,2] (mask [B,H,W,1], default ones) -> the colour-wheel image [B,H,W,3] float32 in [0, 1]:
    hue = direction (the reference's own atan2 table: u == 0 maps to +-pi), saturation = |flow| * 8 / max_flow, value 1, times
    mask.  max_flow None: max |flow * mask| over the batch; given: max(max_flow, 1).  Where the reference yields NaN this gives
    white: a zero vector (saturation 0) and an all-zero field (max_flow 0).  uint8=True: the 8-bit image instead (round to
    nearest)."""
    flow = _dense(flow, 2, 'flow_to_color: flow')
    B, H, W, _ = flow.shape
    mask = None if mask is None else _dense(mask, 1, 'flow_to_color: mask')
    if mask is not None and mask.shape[:3] != flow.shape[:3]:
        raise ValueError("flow_to_color: mask %s does not match flow %s" % (tuple(mask.shape), tuple(flow.shape)))
    out = torch.empty(B, H, W, 3, dtype=torch.uint8 if uint8 else torch.float32, device=flow.device)
    with torch.cuda.device(flow.device):
        mf = None if max_flow is None else ctypes.byref(ctypes.c_float(float(max_flow)))
        bits = torch.zeros(2, dtype=torch.int32, device=flow.device) if max_flow is None else None
        _lib.check(_lib.lib().unflow_flow_to_color(_lib.ptr(flow), _lib.ptr(mask), mf, B, H, W, None if uint8 else _lib.ptr(out),
                                                   _lib.ptr(out) if uint8 else None, _lib.ptr(bits), _lib.stream(flow.device)),
                   "flow_to_color")
    return out


def flow_error_image(flow_1, flow_2, mask_occ, mask_noc=None, log_colors=True, uint8=False):
    """flow_util.py:46-95: the error between flow_1 and flow_2 (the ground truth), [B,H,W,2] each, as an image [B,H,W,3] float32
    in [0, 1].  log_colors: the KITTI devkit's map of min(diff / 3, 20 diff / |gt|) — blue: correct, red: wrong — halved where
    mask_noc == 0 (occluded), black where mask_occ == 0; else min(diff, 5) / 5, red where occluded.  mask_occ, mask_noc
    [B,H,W,1] (mask_noc default ones).  uint8=True: the 8-bit image instead."""
    flow_1, flow_2 = _dense(flow_1, 2, 'flow_error_image: flow_1'), _dense(flow_2, 2, 'flow_error_image: flow_2')
    mask_occ = _dense(mask_occ, 1, 'flow_error_image: mask_occ')
    mask_noc = None if mask_noc is None else _dense(mask_noc, 1, 'flow_error_image: mask_noc')
    B, H, W, _ = flow_1.shape
    for t in (flow_2, mask_occ, mask_noc):
        if t is not None and t.shape[:3] != flow_1.shape[:3]:
            raise ValueError("flow_error_image: shapes differ: %s and %s" % (tuple(flow_1.shape), tuple(t.shape)))
    out = torch.empty(B, H, W, 3, dtype=torch.uint8 if uint8 else torch.float32, device=flow_1.device)
    with torch.cuda.device(flow_1.device):
        _lib.check(_lib.lib().unflow_flow_error_image(_lib.ptr(flow_1), _lib.ptr(flow_2), _lib.ptr(mask_occ), _lib.ptr(mask_noc),
                                                      int(bool(log_colors)), B, H, W, None if uint8 else _lib.ptr(out),
                                                      _lib.ptr(out) if uint8 else None, _lib.stream(flow_1.device)),
                   "flow_error_image")
    return out


def euclidean(t):
    return torch.sqrt((t ** 2).sum(3, keepdim=True))


def outlier_ratio(gt_flow, flow, mask, threshold=3.0, relative=0.05):
    """flow_util.py:106-114."""
    diff = euclidean(gt_flow - flow) * mask
    thr = torch.clamp(euclidean(gt_flow) * relative, min=threshold) if relative is not None else threshold
    return (diff >= thr).float().sum() / mask.sum()


def outlier_pct(gt_flow, flow, mask, threshold=3.0, relative=0.05):
    return outlier_ratio(gt_flow, flow, mask, threshold, relative) * 100
