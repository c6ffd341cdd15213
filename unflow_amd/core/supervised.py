"""Mirror of src/e2eflow/core/supervised.py:12-65: the supervised fine-tuning loss (KITTI ground truth), on the one-direction
engine (core/engine.py, FlowNetEngine(supervised=True))."""
import torch

from .engine import CHANNEL_MEAN, FlowNetEngine

_engines = {}


def get_supervised_engine(batch, height, width, params=None, device=None):
    """One-direction engine per (shape, device, flownet / full_res / train_all), cached like flownet.get_engine."""
    params = params or {}
    ep = {k: params[k] for k in ('flownet', 'full_res', 'train_all', 'gt_sampling') if params.get(k) is not None}
    key = (batch, height, width, None if device is None else str(torch.device(device)), tuple(sorted(ep.items())))
    if key not in _engines:
        _engines[key] = FlowNetEngine(batch, height, width, params=dict(ep, flownet=ep.get('flownet', 'S')), device=device,
                                      supervised=True)
    return _engines[key]


def supervised_loss(batch, params, normalization=None, augment=True, return_flow=False, engine=None, backward=False,
                    generator=None):
    """batch = (im1, im2, flow_gt, mask_gt), NHWC float32, images in [0,255], flow_gt [B,H,W,2], mask_gt [B,H,W,1].
    `normalization` is accepted for signature compatibility; the channel means are the reference's (core/input.py:45).
    augment: True draws random_photometric with the reference's ranges (supervised.py:21-25; host RNG `generator`), a dict
    replays given draws (core.augment.draw_supervised_augmentation; with theta_global / theta_local in it — geometric=True —
    the engine also resamples both frames and the ground truth, params['gt_sampling'] = 'bilinear' or 'nearest'), False/None
    disables it.  With backward=True the
    parameter gradients are left in engine.G.  return_flow: also the final forward flow [B,H,W,2]."""
    if normalization is not None:
        mean = [float(v) for v in normalization[0]]
        if max(abs(a - b) for a, b in zip(mean, CHANNEL_MEAN)) > 1e-3:
            raise NotImplementedError("custom channel means")
    im1, im2, flow_gt, mask_gt = batch
    B, H, W, _ = im1.shape
    eng = engine or get_supervised_engine(B, H, W, params=params, device=getattr(im1, 'device', None))
    if not eng.supervised:
        raise ValueError("supervised_loss needs a one-direction engine (FlowNetEngine(..., supervised=True))")
    if augment is True:
        from .augment import draw_supervised_augmentation
        augment = draw_supervised_augmentation(B, generator)
    eng.set_input(im1, im2, augment=augment or None, target=(flow_gt, mask_gt))
    eng.forward_net()
    loss = eng.forward_loss(with_grad=backward)
    if backward:
        eng.backward_net()
    if not return_flow:
        return loss[0]
    return loss[0], eng.final_flows()[0]
