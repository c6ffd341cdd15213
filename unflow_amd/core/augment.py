"""Mirror of src/e2eflow/core/augment.py (random_affine :7-56, random_photometric :59-110, random_crop :113-134) on
the HIP kernels of csrc/augment.hip.

The random draws are made on the host with a torch.Generator (TF's RNG streams cannot be reproduced; what is
checked against the oracle is the deterministic transform given the draws), the resampling / photometric maths run
on the GPU.  Every function can return the draws it used so a test or a caller can replay them.
"""
import math

import torch

from .. import _lib
from .._lib import check, ptr, stream


def _uniform(n, lo, hi, generator):
    return torch.rand(n, generator=generator, dtype=torch.float32) * (hi - lo) + lo


def affine_theta(tx, ty, rot_deg, scale, flip=None):
    """theta = [[cos,-sin,tx],[sin,cos,ty]] @ diag(scale*flip, scale, 1) (augment.py:31-48).  [B] fp32 host tensors."""
    rad = (rot_deg * math.pi) / 180.0
    sx = scale if flip is None else scale * flip
    c, s = torch.cos(rad), torch.sin(rad)
    row0 = torch.stack([c * sx, -s * scale, tx], 1)
    row1 = torch.stack([s * sx, c * scale, ty], 1)
    return torch.stack([row0, row1], 1).contiguous()


def draw_affine(num_batch, *, max_translation_x=0.0, max_translation_y=0.0, max_rotation=0.0, min_scale=1.0,
                max_scale=1.0, horizontal_flipping=False, generator=None):
    """The draws of augment.py:23-39 -> theta [B,2,3] (host fp32)."""
    tx = _uniform(num_batch, -max_translation_x, max_translation_x, generator)
    ty = _uniform(num_batch, -max_translation_y, max_translation_y, generator)
    rot = _uniform(num_batch, -max_rotation, max_rotation, generator)
    scale = _uniform(num_batch, min_scale, max_scale, generator)
    flip = None
    if horizontal_flipping:
        f = _uniform(num_batch, 0.0, 1.0, generator)
        flip = torch.where(f > 0.5, -torch.ones(num_batch), torch.ones(num_batch))
    return affine_theta(tx, ty, rot, scale, flip)


def transformer(U, theta, out_size=None, out=None, n_samples=None):
    """spatial_transformer.transformer (spatial_transformer.py:19): U [n_u,H,W,C] CUDA NHWC (channel-slice views
    allowed), theta [n_theta,2,3] (host or device).  Output sample b reads U[b % n_u] with theta[b % n_theta]."""
    assert U.is_cuda and U.dtype == torch.float32 and U.dim() == 4 and U.stride(3) == 1
    n_u, H, W, C = U.shape
    ld_u = U.stride(2)
    assert U.stride(1) == W * ld_u and U.stride(0) == H * W * ld_u
    theta = theta.to(device=U.device, dtype=torch.float32).reshape(-1, 6).contiguous()
    B = n_samples or max(n_u, theta.shape[0])
    Ho, Wo = (H, W) if out_size is None else out_size
    if out is None:
        out = torch.empty(B, Ho, Wo, C, dtype=torch.float32, device=U.device)
    ld_o = out.stride(2)
    check(_lib.lib().unflow_stn_affine_fwd(ptr(U), n_u, ld_u, ptr(theta), theta.shape[0], ptr(out), ld_o, B, H, W, C,
                                           Ho, Wo, stream()), "stn_affine")
    return out


def random_affine(tensors, *, max_translation_x=0.0, max_translation_y=0.0, max_rotation=0.0, min_scale=1.0,
                  max_scale=1.0, horizontal_flipping=False, generator=None, theta=None, return_theta=False):
    """augment.random_affine (augment.py:7-56): every tensor of the list gets the same per-sample transform.
    `theta` replays given draws."""
    num_batch = tensors[0].shape[0]
    if theta is None:
        theta = draw_affine(num_batch, max_translation_x=max_translation_x, max_translation_y=max_translation_y,
                            max_rotation=max_rotation, min_scale=min_scale, max_scale=max_scale,
                            horizontal_flipping=horizontal_flipping, generator=generator)
    out = [transformer(t, theta) for t in tensors]
    return (out, theta) if return_theta else out


def draw_photometric(num_batch, *, noise_stddev=0.0, min_contrast=0.0, max_contrast=0.0, brightness_stddev=0.0,
                     min_colour=1.0, max_colour=1.0, min_gamma=1.0, max_gamma=1.0, generator=None):
    """The draws of augment.py:78-91 (noise and brightness are ONE value per sample, shape [num_batch,1])."""
    d = dict(contrast=_uniform(num_batch, min_contrast, max_contrast, generator),
             gamma=_uniform(num_batch, min_gamma, max_gamma, generator),
             colour=_uniform(num_batch * 3, min_colour, max_colour, generator).view(num_batch, 3))
    z = torch.zeros(num_batch)
    d['noise'] = torch.randn(num_batch, generator=generator) * noise_stddev if noise_stddev > 0.0 else z
    d['brightness'] = torch.randn(num_batch, generator=generator) * brightness_stddev if brightness_stddev > 0.0 \
        else z.clone()
    return d


def photometric(im, draws, out=None, mean=None):
    """The deterministic part of random_photometric (augment.py:93-108) for one image batch [N,H,W,>=3 stride]."""
    assert im.is_cuda and im.dtype == torch.float32 and im.dim() == 4
    N, H, W, _ = im.shape
    dev = im.device
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.float32, device=dev)
    g = {k: v.to(device=dev, dtype=torch.float32).contiguous() for k, v in draws.items()}
    n_par = g['contrast'].numel()
    mean_host = None if mean is None else (_lib.ctypes.c_float * 3)(*[float(v) for v in mean])
    check(_lib.lib().unflow_photometric_augment(ptr(im), im.stride(2), ptr(out), out.stride(2), ptr(g['contrast']),
                                                ptr(g['brightness']), ptr(g['colour']), ptr(g['gamma']),
                                                ptr(g['noise']), n_par, mean_host, N, H, W, stream()), "photometric")
    return out


def random_photometric(ims, *, noise_stddev=0.0, min_contrast=0.0, max_contrast=0.0, brightness_stddev=0.0,
                       min_colour=1.0, max_colour=1.0, min_gamma=1.0, max_gamma=1.0, generator=None, draws=None,
                       return_draws=False):
    """augment.random_photometric (augment.py:59-110): ims = list of [B,H,W,3] batches in [0,1]."""
    if draws is None:
        draws = draw_photometric(ims[0].shape[0], noise_stddev=noise_stddev, min_contrast=min_contrast,
                                 max_contrast=max_contrast, brightness_stddev=brightness_stddev,
                                 min_colour=min_colour, max_colour=max_colour, min_gamma=min_gamma,
                                 max_gamma=max_gamma, generator=generator)
    out = [photometric(im, draws) for im in ims]
    return (out, draws) if return_draws else out


def random_crop(tensors, size, seed=None, name=None):
    """augment.random_crop (augment.py:113-134): the same random window of `size` (full-rank, like tf.slice) from
    every tensor; with two tensors the limit is the elementwise minimum of their shapes."""
    g = None
    if seed is not None:
        g = torch.Generator().manual_seed(int(seed))
    shape = list(tensors[0].shape)
    if len(tensors) == 2:
        shape = [min(a, b) for a, b in zip(tensors[0].shape, tensors[1].shape)]
    offset = [int(torch.randint(0, s - z + 1, (1,), generator=g)) for s, z in zip(shape, size)]
    sl = tuple(slice(o, o + z) for o, z in zip(offset, size))
    return [t[sl] for t in tensors]


def draw_training_augmentation(num_batch, generator=None):
    """All draws of one training step, with the reference's ranges (unsupervised.py:39-58)."""
    aug = dict(theta_global=draw_affine(num_batch, horizontal_flipping=True, min_scale=0.9, max_scale=1.1,
                                        generator=generator),
               theta_local=draw_affine(num_batch, min_scale=0.9, max_scale=1.1, generator=generator))
    aug.update(draw_photometric(num_batch, noise_stddev=0.04, min_contrast=-0.3, max_contrast=0.3,
                                brightness_stddev=0.02, min_colour=0.9, max_colour=1.1, min_gamma=0.7,
                                max_gamma=1.5, generator=generator))
    return aug


# Range keys of the geometric part of draw_supervised_augmentation (draw_affine's keywords; 'local_' + key: the local transform
# of the second frame).  Trainer reads them from params as 'augment_' + key.
GEOMETRIC_RANGE_KEYS = ('max_translation_x', 'max_translation_y', 'max_rotation', 'min_scale', 'max_scale', 'horizontal_flipping',
                        'local_max_translation_x', 'local_max_translation_y', 'local_max_rotation', 'local_min_scale',
                        'local_max_scale')


def draw_supervised_augmentation(num_batch, generator=None, geometric=False, **ranges):
    """The draws of the supervised step (supervised.py:21-25): photometric only, the same ranges as the photometric part of
    draw_training_augmentation; one draw per image pair, applied to both frames.
    geometric=True (this project's addition): the dict also carries theta_global and theta_local of draw_affine, by
    default with the unsupervised step's ranges (unsupervised.py:39-50: global = flip and scale 0.9 .. 1.1, local = scale
    0.9 .. 1.1); `ranges` overrides them (GEOMETRIC_RANGE_KEYS).  The photometric draws come FIRST, so a seed gives the same
    photometric draws with and without `geometric`."""
    unknown = sorted(set(ranges) - set(GEOMETRIC_RANGE_KEYS))
    if unknown or (ranges and not geometric):
        raise TypeError("draw_supervised_augmentation: %s" % ("unknown range keys %s" % unknown if unknown else
                                                              "range keys need geometric=True"))
    aug = draw_photometric(num_batch, noise_stddev=0.04, min_contrast=-0.3, max_contrast=0.3, brightness_stddev=0.02,
                           min_colour=0.9, max_colour=1.1, min_gamma=0.7, max_gamma=1.5, generator=generator)
    if geometric:
        glob = dict(horizontal_flipping=True, min_scale=0.9, max_scale=1.1)
        loc = dict(min_scale=0.9, max_scale=1.1)
        for k, v in ranges.items():
            if k.startswith('local_'):
                loc[k[len('local_'):]] = v
            else:
                glob[k] = v
        aug['theta_global'] = draw_affine(num_batch, generator=generator, **glob)
        aug['theta_local'] = draw_affine(num_batch, generator=generator, **loc)
    return aug


def identity_photometric(num_batch):
    """Photometric draws that change nothing: contrast 0, brightness 0, colour 1, gamma 1, noise 0."""
    z = torch.zeros(num_batch)
    return dict(contrast=z.clone(), brightness=z.clone(), colour=torch.ones(num_batch, 3), gamma=torch.ones(num_batch), noise=z)


def pixel_identity_theta(H, W):
    """The theta whose PIXEL map is the identity: [(W-1)/W, 0, -1/W, 0, (H-1)/H, -1/H] (not theta = I: the transformer's
    normalised grid spans [-1, 1] over W - 1 steps but is scaled back by W / 2).  [1,2,3] float64."""
    return torch.tensor([[[(W - 1) / W, 0.0, -1.0 / W], [0.0, (H - 1) / H, -1.0 / H]]], dtype=torch.float64)


def affine_pixel_matrix(theta, H, W):
    """A(theta; H, W): the map of transformer() from output pixel (px, py) to the source coordinate, as [B,3,3] float64 on
    (px, py, 1):  x = (W/2) (t0 (2 px / (W-1) - 1) + t1 (2 py / (H-1) - 1) + t2 + 1), y likewise with H/2 and t3..t5."""
    if H < 2 or W < 2:
        raise ValueError("affine_pixel_matrix: the transformer's grid needs H, W >= 2, got %d x %d" % (H, W))
    t = torch.as_tensor(theta).detach().to('cpu', torch.float64).reshape(-1, 6)
    A = torch.zeros(t.shape[0], 3, 3, dtype=torch.float64)
    A[:, 0, 0] = W * t[:, 0] / (W - 1)
    A[:, 0, 1] = W * t[:, 1] / (H - 1)
    A[:, 0, 2] = (W / 2.0) * (-t[:, 0] - t[:, 1] + t[:, 2] + 1.0)
    A[:, 1, 0] = H * t[:, 3] / (W - 1)
    A[:, 1, 1] = H * t[:, 4] / (H - 1)
    A[:, 1, 2] = (H / 2.0) * (-t[:, 3] - t[:, 4] + t[:, 5] + 1.0)
    A[:, 2, 2] = 1.0
    return A


def affine_pixel_maps(theta_global, theta_local, H, W, dtype=torch.float32):
    """The three pixel maps of unflow_supervised_geo_augment per sample, formed in fp64 and rounded once: [B,3,6] =
    (M1 = G, M2 = G L, M2^-1) with G = A(theta_global), L = A(theta_local) — the unsupervised step shows im1(G p) and
    im2(G (L p)) (engine.set_input's chain) — each as the two rows [a b c; d e f] of the affine 3 x 3."""
    G, L = affine_pixel_matrix(theta_global, H, W), affine_pixel_matrix(theta_local, H, W)
    if G.shape[0] != L.shape[0]:
        raise ValueError("affine_pixel_maps: %d global and %d local thetas" % (G.shape[0], L.shape[0]))
    M2 = G @ L
    M2i = torch.linalg.inv(M2)
    return torch.stack([G[:, :2], M2[:, :2], M2i[:, :2]], 1).reshape(-1, 3, 6).to(dtype).contiguous()


GT_SAMPLING = {'bilinear': 0, 'nearest': 1}


def supervised_geo_augment(im1, im2, flow_gt, mask_gt, mats, draws, im01, x0, flow_out, mask_out, gt_sampling='bilinear',
                           mean=None):
    """unflow_supervised_geo_augment (csrc/augment_flow.hip): im1, im2 [B,H,W,3] in [0,255], flow_gt [B,H,W,2], mask_gt
    [B,H,W,1] or None, mats = affine_pixel_maps(...) -> im01 [2B,H,W,3], x0 [2B,H,W,>=3 stride], flow_out [B,H,W,2],
    mask_out [B,H,W,1], all written in one launch.  draws: photometric draws (identity_photometric for none)."""
    if gt_sampling not in GT_SAMPLING:
        raise ValueError("gt_sampling must be one of %s, got %r" % (sorted(GT_SAMPLING), gt_sampling))
    B, H, W, _ = im1.shape
    dev = im1.device
    for t, shape in ((im1, (B, H, W, 3)), (im2, (B, H, W, 3)), (flow_gt, (B, H, W, 2)), (im01, (2 * B, H, W, 3)),
                     (flow_out, (B, H, W, 2)), (mask_out, (B, H, W, 1))) + (() if mask_gt is None else ((mask_gt, (B, H, W, 1)),)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, (tuple(t.shape), shape)
    assert x0.is_cuda and x0.dtype == torch.float32 and x0.stride(3) == 1 and tuple(x0.shape[:3]) == (2 * B, H, W)
    ld = x0.stride(2)
    assert x0.stride(1) == W * ld and x0.stride(0) == H * W * ld
    mats = torch.as_tensor(mats).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(mats.shape) != (B, 3, 6):
        raise ValueError("supervised_geo_augment: mats must be [%d,3,6], got %s" % (B, tuple(mats.shape)))
    g = {k: draws[k].to(device=dev, dtype=torch.float32).contiguous() for k in ('contrast', 'brightness', 'colour', 'gamma', 'noise')}
    mean_host = None if mean is None else (_lib.ctypes.c_float * 3)(*[float(v) for v in mean])
    check(_lib.lib().unflow_supervised_geo_augment(
        ptr(im1), ptr(im2), ptr(flow_gt), ptr(mask_gt), ptr(mats), ptr(g['contrast']), ptr(g['brightness']), ptr(g['colour']),
        ptr(g['gamma']), ptr(g['noise']), g['contrast'].numel(), mean_host, ptr(im01), ptr(x0), ld, ptr(flow_out), ptr(mask_out),
        GT_SAMPLING[gt_sampling], B, H, W, stream()), "supervised_geo_augment")
