"""Forward-only flow inference: what a user does with a trained model — flow for new frames, a checkpoint scored on KITTI,
files for the benchmark (the non-GUI part of the reference's src/eval_gui.py).

FlowEstimator owns one forward-only engine (FlowNetEngine(..., inference=True)), fixed device staging buffers, a device
table of per-sample frame geometry and one captured hipGraph on one stream:

    unflow_inference_input   staged frames (uint8 or fp32, any size up to max_frame) -> network input (+ conv1's planes)
    engine.forward_net()
    unflow_inference_output  flow2 -> frame-size flow [B][Hmax][Wmax][2], its KITTI 16-bit encoding, EPE / outlier sums

Every batch — any mix of frame sizes, a short last one — replays the same graph: the host rewrites the geometry table
(csrc/inference.hip).  Host staging is double-buffered in pinned memory; before the host overwrites a slot it waits for the
event recorded after the last replay that read it (and the copies that brought its outputs back).

bidirectional=True: the engine runs both directions (FlowNetEngine(..., inference=True, bidirectional=True)) and the graph
continues with the output kernel once more on the backward rows (no ground truth) and

    unflow_inference_occlusion   both frame-size flows -> losses.occlusion's masks of both directions, integer TP / FP / FN
                                 of the forward mask against KITTI's occluded pixels

visual=True: the graph ends with the pictures of eval_gui.py's window (csrc/visual.hip), as 8-bit images:

    unflow_inference_visual      staged frames, frame-size flow, staged ground truth -> overlay, brightness error, flow colours,
                                 and with ground truth the KITTI error image and the ground truth's colours

sequence=True: flow along a clip f0 .. fT-1, every frame uploaded once and encoded once.  The engine
(FlowNetEngine(..., inference=True, sequence=True)) keeps F = B + 1 frame rows, pair i = (row i, row i + 1), and the graph is

    unflow_sequence_carry          row `src` (the previous replay's last frame) -> row 0 of the input and of the tower's outputs
    unflow_inference_input_frames  up to B new staged frames -> rows [1, F)
    engine.forward_net()
    unflow_inference_output        driven by a per-PAIR table: a slot whose two rows do not both hold frames of the clip has h = 0

with the frame table, the pair table and src in one device int32 buffer the host rewrites before each replay (push,
estimate_sequence, export_sequence; sequence_tables is the host packing).

sequence='bidirectional': both of the above along a clip.  The engine keeps the same F frame rows and tower and
runs everything behind the tower on 2B rows, a block of B backward pairs (frame i + 1, frame i) and a block of B forward pairs;
unflow_sequence_mirror, inside forward_net() behind conv2, gives the backward block's decoder the skip connection of ITS first
frame.  The graph ends with unflow_inference_output on either block and unflow_inference_occlusion, all over the pair table
(push_bidirectional, estimate_sequence_bidirectional, export_sequence(backward=, occlusion=)).

sequence=True | 'bidirectional' with visual='sequence': pictures along a clip (visual=True is the pair estimator's
flag and, with sequence, still a ValueError that names this spelling).  Either sequence graph ends with

    unflow_sequence_visual         the new staged frames -> one shown frame per engine row, each frame of the clip resampled once
                                   (row 0 carried like the engine's); per pair of the pair table the overlay, the brightness
                                   error and the flow colours of unflow_inference_visual; bidirectional: also the backward flow's
                                   colours and the brightness error of the non-occluded pixels

(push_visual, visualize_sequence, export_sequence(visual=True)); a clip-wide max_flow of the colours travels in the tables.

sequence=True | 'bidirectional' with track=True | S | anchors: tracks along a clip.  Behind the output (and
occlusion) kernels either sequence graph runs

    unflow_sequence_track          the forward flows of the replay's pairs (bidirectional: and the forward occlusion masks) -> per
                                   pair, where every anchor of the clip's first frame is now and whether it is still visible; the
                                   state (displacement, alive) stays on the device from one replay of the clip to the next

(push_tracks, track_sequence, export_sequence(tracks=True)); the grid stride and the number of tracks travel in the tables.

sequence=True | 'bidirectional' with interpolate=n: n in-between frames per pair.  Behind the output (and occlusion,
and track) kernels either sequence graph runs

    unflow_sequence_interpolate    the staged frames, the forward flow (bidirectional: and the backward flow and both occlusion
                                   masks) -> per pair n motion-compensated frames, an integer splat normalised by its weight, and
                                   the count of the holes; the clip's last staged frame stays on the device for the next replay

(push_interpolated, interpolate_sequence, export_sequence(interpolate=True)).  With interpolate_order=k the graph runs
unflow_sequence_interpolate_ordered(..., k) in its place, on the same buffers: the splat weighted by how well the two frames agree
along each pixel's flow.  Everything on top is unchanged.

sequence=True | 'bidirectional' with ground_truth=True: scores along a clip.  The ground truth of every pair is staged
per pair slot, the pair table carries its number of maps, the output kernel on the forward rows scores it (the occlusion kernel
counts TP / FP / FN with two maps), and with track the graph runs, behind unflow_sequence_track,

    unflow_sequence_track_score    the staged ground-truth flow and masks of the replay's pairs -> ground-truth tracks, chained as
                                   the tracks are and ended at invalid (two maps: or occluded) pixels, and per pair the integer
                                   counts and the fp64 error sum of this replay's tracks against them; the ground-truth state stays
                                   on the device from one replay of the clip to the next

(push_scored, evaluate_sequence).

sequence=True | 'bidirectional' with interpolate=n and held_out=True: the in-between frames scored against held-out frames (DESIGN
7.18).  The frames that were left out of the clip are staged per pair slot and j, the pair table says `held`, and behind
unflow_sequence_interpolate the graph runs

    unflow_sequence_interpolate_score   the staged frames, out_mid and the truth frames -> per pair, j and candidate (the interpolated
                                   frame, the temporal blend, the nearest frame) the exact squared error and the sum of the 8 x 8
                                   window SSIMs, reduced in a fixed order; its own copy of the clip's last frame stays on the device

(push_held_out, evaluate_interpolation).

sequence=True | 'bidirectional' with stabilise=True | dict(tol, iters, follow): camera motion along a clip.  Behind the
track kernels and in front of the interpolation either sequence graph runs

    unflow_sequence_stabilise      the forward flow of the replay's pairs (bidirectional: and the forward occlusion mask) -> per pair
                                   a robust affine fit (integer sums, one fp64 solve per iteration on the device), every pixel's
                                   residual against it, the camera path composed along the clip, and the staged later frame
                                   resampled along that path; the path stays on the device from one replay of the clip to the next

(push_stabilised, stabilise_sequence, export_sequence(stabilise=True)); tol, iters and follow travel by value.

sequence='bidirectional' with denoise=True | dict(tol, depth): temporal denoising along a clip.  Behind
unflow_inference_occlusion the bidirectional sequence graph runs

    unflow_sequence_denoise        the staged frames, the backward flow and the backward occlusion mask of the replay's pairs -> per
                                   pair the later frame averaged with its own history fetched along the backward flow (a gather,
                                   integers throughout); the history stays on the device from one replay of the clip to the next

(push_denoised, denoise_sequence, export_sequence(denoise=True)); tol and depth travel by value.

The host side is the same for every mode.  output_buffers lists what a replay can bring back (device buffer, pinned copy, flag);
_submit / _submit_sequence stage their inputs and end in _replay (run, copy back, the files' scanlines, the slot's event), which
leaves the replay's rows [(slot row, h, w)] in slot.pending; _one_ahead keeps one replay in flight ahead of the caller; pair_files
is the list of files of a pair, and _write_files the one loop that writes them, on the host or through the writer pool.  A new
output is a row of output_buffers, a new file kind a row of pair_files and a branch of _write_files.
"""
import collections
import contextlib
import itertools
import math
import os

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from .engine import FLOW_SCALE, FlowNetEngine

ENGINE_KEYS = ('flownet', 'train_all', 'full_res', 'pyramid_loss', 'border_mask', 'mask_occlusion')   # = Trainer.ENGINE_KEYS
MAP_NAMES = {2: ('occluded', 'non-occluded'), 1: ('all',)}
OCC_NAMES = ('occ/precision', 'occ/recall', 'occ/F1')
_UNSET = object()

# What estimate_bidirectional returns per pair: [h, w, 2] float32 flows, [h, w] bool occlusion masks (losses.occlusion)
BidirectionalFlow = collections.namedtuple('BidirectionalFlow', ('flow_fw', 'flow_bw', 'occ_fw', 'occ_bw'))
# What visualize returns per pair: uint8 [h, w, 3] images — eval_gui.py:199-204's slots (the overlay in place of the first image)
FlowVisual = collections.namedtuple('FlowVisual', ('overlay', 'warp_error', 'flow'))
# The images of unflow_inference_visual, in its order, and the file each is exported to (%06d_<tag>.png)
VISUAL_IMAGES = ('overlay', 'warp_error', 'flow', 'error', 'gt')
VISUAL_TAGS = ('img', 'diff', 'flow', 'err', 'gt')


def visual_files(n, has_gt):
    """The picture files of example n, in the order they are written: [(index into VISUAL_IMAGES, file name)]."""
    return [(k, '%06d_%s.png' % (n, VISUAL_TAGS[k])) for k in (0, 2, 1) + ((3, 4) if has_gt else ())]


# What visualize_sequence returns per pair of a sequence='bidirectional' estimator: FlowVisual's three, the backward flow's colours
# and the brightness error where the forward occlusion mask is 0 — the images of unflow_sequence_visual, in its order
SequenceVisual = collections.namedtuple('SequenceVisual', FlowVisual._fields + ('flow_bw', 'warp_error_noc'))
SEQUENCE_VISUAL_TAGS = VISUAL_TAGS[:3] + ('flow_bw', 'diff_noc')


def sequence_visual_files(n, bidirectional):
    """The picture files of pair n of a clip, in the order they are written: [(image of unflow_sequence_visual, file name)]."""
    return [(k, '%06d_%s.png' % (n, SEQUENCE_VISUAL_TAGS[k])) for k in (0, 2, 1) + ((3, 4) if bidirectional else ())]


# What push_tracks returns per pair (n, n + 1): disp float32, where every anchor of the clip's first frame is in frame n + 1, as
# its displacement from the anchor, and alive bool, still in the frame and never occluded — [gh, gw, 2] and [gh, gw] for the dense
# grid, [N, 2] and [N] for sparse anchors
Track = collections.namedtuple('Track', ('disp', 'alive'))
# What push_interpolated returns per pair (n, n + 1): frames uint8 [n_mid, h, w, 3], the in-between frames j = 1..n_mid at time
# j / (n_mid + 1), and holes int [n_mid], the pixels of each that no source reached (filled with the temporal blend)
Interpolated = collections.namedtuple('Interpolated', ('frames', 'holes'))
# What push_held_out returns per pair: Interpolated's frames and holes, then per in-between frame j and candidate kind (MID_KINDS:
# the interpolated frame, the temporal blend, the nearest frame) against the held-out frame: sse int64 [n_mid, 3], the summed squared
# byte error; psnr [n_mid, 3] = 10 log10(255^2 3 h w / sse), inf at sse = 0; ssim [n_mid, 3], the mean 8 x 8-window SSIM over the 3
# (h - 7)(w - 7) windows, nan without a window
HeldOut = collections.namedtuple('HeldOut', ('frames', 'holes', 'sse', 'psnr', 'ssim'))
MID_KINDS = ('mid', 'blend', 'nearest')


def mid_windows(h, w):
    """The 8 x 8 window positions of an (h, w) frame times its 3 channels: what a pair's SSIM sum is divided by."""
    return 3 * max(int(h) - 7, 0) * max(int(w) - 7, 0)


def mid_psnr(sse, values):
    """10 log10(255^2 values / sse) of integer squared-error sums over `values` byte values; inf where sse = 0."""
    sse = np.asarray(sse, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(255.0 ** 2 * float(values) / sse)


def mid_mean_ssim(ssim_sum, windows):
    """SSIM sums over `windows` windows as means; nan without a window."""
    ssim_sum = np.asarray(ssim_sum, dtype=np.float64)
    return ssim_sum / float(windows) if windows else np.full(ssim_sum.shape, np.nan)
# What push_scored returns per pair: the flow, then per map of the ground truth aee, outliers (%) and mask_sum (the scored pixels);
# occ_counts [tp, fp, fn] (both directions and two maps) or None; track a TrackScore (an estimator with track) or None
PairScore = collections.namedtuple('PairScore', ('flow', 'aee', 'outliers', 'mask_sum', 'occ_counts', 'track'))
# A pair's tracks against the chained ground truth (unflow_sequence_track_score): the counts of live ground-truth, predicted and
# both-alive tracks; epe, the mean distance over the both-alive ones; per threshold 1, 2, 4, 8, 16 px pos_acc (ground-truth-alive
# tracks within it, a dead prediction's frozen position counting) and jaccard (both alive and within it, over either alive);
# occ_acc, the tracks whose alive flag agrees; the ground-truth tracks themselves, shaped as Track's
TrackScore = collections.namedtuple('TrackScore', ('n_gt', 'n_pred', 'n_both', 'epe', 'pos_acc', 'jaccard', 'occ_acc', 'gt_disp',
                                                   'gt_alive'))
TRACK_SCORE_THRESHOLDS = (1.0, 2.0, 4.0, 8.0, 16.0)      # px; the kernel compares the squared distance with their squares


def track_score(words, err, gt_disp, gt_alive):
    """The 16 integer words and the error sum of unflow_sequence_track_score (one slot, or several summed) as a TrackScore; a
    ratio whose denominator is 0 is nan."""
    w = [int(v) for v in words]
    ratio = lambda a, b: a / b if b else float('nan')          # noqa: E731
    n_gt, n_pred, n_both = w[:3]
    return TrackScore(n_gt, n_pred, n_both, ratio(float(err), n_both), [ratio(w[3 + k], n_gt) for k in range(5)],
                      [ratio(w[8 + k], n_gt + n_pred - w[8 + k]) for k in range(5)], ratio(w[13], w[14]), gt_disp, gt_alive)


TRACK_DEAD = 1e10         # a dead track in %06d_track.flo: the .flo unknown-flow convention (read back as mask = 0)


def track_option(track):
    """FlowEstimator's track option -> None (no tracks), ('dense', S): the grid of stride S over the frame (True: S = 1), or
    ('sparse', int32 [N, 2] array of (x, y) anchors).  Anything else: ValueError."""
    if track is None or track is False:
        return None
    if track is True:
        return ('dense', 1)
    if isinstance(track, (int, np.integer)):
        if int(track) < 1:
            raise ValueError("FlowEstimator: track=S is a grid stride >= 1, got %d" % int(track))
        return ('dense', int(track))
    if isinstance(track, (str, bytes, dict)):
        raise ValueError("FlowEstimator: track is True, a grid stride S >= 1 or an int array [N][2] of (x, y) anchors, got %r"
                         % (track,))
    try:
        a = np.asarray(track.cpu().numpy() if isinstance(track, torch.Tensor) else track)
    except Exception:
        a = None
    if a is None or a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("FlowEstimator: track is True, a grid stride S >= 1 or an int array [N][2] of (x, y) anchors, got %s"
                         % ("%s %s" % (a.dtype, a.shape) if a is not None else repr(track)))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("FlowEstimator: track anchors are int32 pixel coordinates")
    return ('sparse', np.ascontiguousarray(a, dtype=np.int32))


def track_grid(shape, stride):
    """(gh, gw) of the dense anchor grid of that stride over a frame of shape (h, w): anchors (stride * gx, stride * gy)."""
    return (-(-int(shape[0]) // int(stride)), -(-int(shape[1]) // int(stride)))


def interpolate_option(interpolate):
    """FlowEstimator's interpolate option -> the number of in-between frames per pair: 0 (None or False: none) or an int n in
    1..7.  Anything else: ValueError."""
    if interpolate is None or interpolate is False:
        return 0
    if isinstance(interpolate, bool) or not isinstance(interpolate, (int, np.integer)) or not 1 <= int(interpolate) <= 7:
        raise ValueError("FlowEstimator: interpolate=n is an int, 1 to 7 in-between frames per pair, got %r" % (interpolate,))
    return int(interpolate)


def interpolate_order_option(interpolate_order, interpolate=1):
    """FlowEstimator's interpolate_order option -> the order of unflow_sequence_interpolate_ordered: 0 (None or 0: the plain
    entry) or an int k in 1..4, the steepness of the consistency weight.  Anything else, or a k without in-between
    frames (interpolate: interpolate_option's number), is a ValueError."""
    if interpolate_order is None:
        return 0
    if isinstance(interpolate_order, bool) or not isinstance(interpolate_order, (int, np.integer)) or not 0 <= int(interpolate_order) <= 4:
        raise ValueError("FlowEstimator: interpolate_order=k is an int, 1 to 4 (None or 0: unordered), got %r" % (interpolate_order,))
    if int(interpolate_order) and not interpolate:
        raise ValueError("FlowEstimator: interpolate_order orders the splat of the in-between frames; it needs interpolate=n")
    return int(interpolate_order)


# What push_stabilised returns per pair (n, n + 1) (unflow_sequence_stabilise): frame uint8 [h, w, 3], frame n + 1
# resampled along the camera path (uncovered pixels black); residual uint8 [h, w], how far every pixel's flow is from the pair's
# dominant motion, in quarter pixels of L1 distance (255: that or more, or no usable flow); motion int64 [8] = {Tu, Lux, Luy, Tv,
# Lvx, Lvy, status | successful iterations << 8, pixels used}, the affine fit, T in 2^-16 px, L in 2^-24 per pixel; path int64 [8],
# the path after the pair in the same units (its linear part includes the identity); counts int64 [4] = {valid, valid but occluded,
# moving, uncovered} pixels.  camera_matrix turns motion or path into a 2 x 3 matrix.
Stabilised = collections.namedtuple('Stabilised', ('frame', 'residual', 'motion', 'path', 'counts'))
STABILISE_DEFAULTS = dict(tol=2, iters=3, follow=0)
STABILISE_RANGES = dict(tol=(0, 4), iters=(0, 4), follow=(0, 8))


def stabilise_option(stabilise):
    """FlowEstimator's stabilise option -> None (None or False: no camera motion) or dict(tol, iters, follow): True gives
    STABILISE_DEFAULTS, a dict overrides some of them — tol in 0..4 (the weight of a pixel halves per 2^(1 - tol) px of residual),
    iters in 0..4 (reweighted fits behind the first), follow in 0..8 (0: lock, every frame in the first frame's coordinates; s: the
    path loses 2^-s of its offset per pair).  Anything else: ValueError."""
    if stabilise is None or stabilise is False:
        return None
    if stabilise is True:
        return dict(STABILISE_DEFAULTS)
    if not isinstance(stabilise, dict) or set(stabilise) - set(STABILISE_DEFAULTS):
        raise ValueError("FlowEstimator: stabilise is True or a dict with tol, iters, follow, got %r" % (stabilise,))
    out = dict(STABILISE_DEFAULTS)
    for key, v in stabilise.items():
        lo, hi = STABILISE_RANGES[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("FlowEstimator: stabilise['%s'] is an int in %d..%d, got %r" % (key, lo, hi, v))
        out[key] = int(v)
    return out


def camera_matrix(words, h, w, path=False):
    """Six words of a Stabilised tuple as a float64 2 x 3 matrix A in pixel coordinates, (x', y') = A (x, y, 1).  motion (path
    False): where the dominant motion takes a pixel of frame n in frame n + 1, p + T + L (p - c).  path (True): where a pixel of
    the stabilised frame is in frame n + 1, c + Dt + Dl (p - c).  c = ((w - 1) / 2, (h - 1) / 2)."""
    v = [int(x) for x in np.asarray(words).reshape(-1)[:6]]
    lin = np.array([[v[1], v[2]], [v[4], v[5]]], dtype=np.float64) / float(1 << 24)
    if not path:
        lin = lin + np.eye(2)
    c = np.array([(int(w) - 1) / 2.0, (int(h) - 1) / 2.0])
    t = c + np.array([v[0], v[3]], dtype=np.float64) / 65536.0 - lin @ c
    return np.concatenate([lin, t[:, None]], axis=1)


# What push_denoised returns per pair (n, n + 1) (unflow_sequence_denoise): frame uint8 [h, w, 3], frame n + 1
# averaged with its history along the backward flow; noise, the pair's noise level M (the median over the pixels with a history of
# the L1 distance, three channels summed, between the frame and its prediction, in grey levels, at most 255); tol, the tolerance
# 0..4 the pair was filtered with (the chosen one with tol='auto'); counts, a dict: eligible (pixels with a history), fresh (pixels
# without: no usable flow, a source outside the frame, or occluded), rejected (pixels whose history was too far from the frame and
# was dropped) and history, the mean history count behind the pair (1: nothing averaged, up to depth).
Denoised = collections.namedtuple('Denoised', ('frame', 'noise', 'tol', 'counts'))
DENOISE_DEFAULTS = dict(tol='auto', depth=8)
DENOISE_RANGES = dict(tol=(0, 4), depth=(1, 64))


def denoise_option(denoise):
    """FlowEstimator's denoise option -> None (None or False: no denoising) or dict(tol, depth): True gives DENOISE_DEFAULTS, a dict
    overrides some of them — tol 'auto' (per pair, from its noise level) or an int in 0..4 (a pixel's history counts half per
    8 * 2^tol grey levels of L1 distance between it and the frame, and not at all from six halvings on), depth in 1..64 (the
    largest history count: the longest average).  Anything else: ValueError."""
    if denoise is None or denoise is False:
        return None
    if denoise is True:
        return dict(DENOISE_DEFAULTS)
    if not isinstance(denoise, dict) or set(denoise) - set(DENOISE_DEFAULTS):
        raise ValueError("FlowEstimator: denoise is True or a dict with tol, depth, got %r" % (denoise,))
    out = dict(DENOISE_DEFAULTS)
    for key, v in denoise.items():
        lo, hi = DENOISE_RANGES[key]
        if key == 'tol' and isinstance(v, str) and v == 'auto':
            out[key] = v
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("FlowEstimator: denoise['%s'] is %san int in %d..%d, got %r"
                             % (key, "'auto' or " if key == 'tol' else '', lo, hi, v))
        out[key] = int(v)
    return out


def pair_files(n, fmt, backward=False, occlusion=False, pictures=(), track=False, mid=0, stab=False, den=False):
    """The files export / export_sequence write for pair n, in the order they are written — _10, _01, _10_occ, then the pictures
    (visual_files' or sequence_visual_files' list) in their file order: [(file name, source)].  A source is

        ('png', surface, k)   a PNG of image k * B + i of the encode surface of that name for row i of the replay (_Encoder; also
                              the slot's pinned copy of it): 'u16', 'u16_bw', 'occ' with k = 0, 'vis' with the picture's index;
        ('flo', attribute)    a .flo file of row i of that pinned flow of the slot: 'flow', 'flow_bw';
        ('track', attribute)  track: the dense tracks of row i on their grid, %06d_track.flo (FlowEstimator._track_flo), last.

    mid: the in-between frames j = 1..mid of the pair, %06d_mid%d.png (pair, j), PNGs of image (j - 1) * B + i of the surface
    'mid', behind the pictures.  stab: the stabilised frame and the residual map of the pair, %06d_stab.png (8-bit RGB, surface
    'stab') and %06d_motion.png (8-bit grey, surface 'stab_resid'), behind those.  den: the denoised frame of the pair,
    %06d_den.png (8-bit RGB, surface 'den'), behind everything else.

    Both back ends of FlowEstimator._write_files and the entries of the replay's unflow_png_filter launch (filter_entries) come
    from this one list, so the span order and the file order cannot drift apart."""
    flows = [('10', 'u16', 'flow')] + ([('01', 'u16_bw', 'flow_bw')] if backward else [])
    out = [('%06d_%s.%s' % (n, tag, fmt), ('png', u16, 0) if fmt == 'png' else ('flo', flow)) for tag, u16, flow in flows]
    if occlusion:
        out.append(('%06d_10_occ.png' % n, ('png', 'occ', 0)))
    return out + [(name, ('png', 'vis', k)) for k, name in pictures] + \
        [('%06d_mid%d.png' % (n, j), ('png', 'mid', j - 1)) for j in range(1, int(mid) + 1)] + \
        ([('%06d_track.flo' % n, ('track', 'track_disp'))] if track else []) + \
        ([('%06d_stab.png' % n, ('png', 'stab', 0)), ('%06d_motion.png' % n, ('png', 'stab_resid', 0))] if stab else []) + \
        ([('%06d_den.png' % n, ('png', 'den', 0))] if den else [])


def filter_entries(files, rows, batch):
    """_filter's entries [(surface name, image, h, w)] of the PNGs among `files` (pair_files' list of one pair; the names do not
    matter) for every row (i, h, w) of a replay of `batch` rows, in the order the files are written."""
    return [(src[1], src[2] * batch + i, h, w) for i, h, w in rows for _, src in files if src[0] == 'png']


def occlusion_scores(counts):
    """This project's KITTI occlusion scores (the reference prints none): the forward occlusion mask against KITTI's occluded
    pixels — evaluated where mask_occ = 1, positive where mask_noc = 0 as well.  counts: per-example [tp, fp, fn]; pooled over
    all examples from the summed counts: precision tp / (tp + fp), recall tp / (tp + fn), F1 2 tp / (2 tp + fp + fn), in %,
    0 where a denominator is 0."""
    tp, fp, fn = (int(v) for v in np.asarray(counts, dtype=np.int64).reshape(-1, 3).sum(0))
    pct = lambda a, b: 100.0 * a / b if b else 0.0          # noqa: E731
    return dict(zip(OCC_NAMES, (pct(tp, tp + fp), pct(tp, tp + fn), pct(2 * tp, 2 * tp + fp + fn))))


# ------------------------------------------------------------------------------------------------- host batch packing
def frame_origin(n, staged):
    """Where a frame of size n starts in a staged axis of size `staged` that holds resize_image_with_crop_or_pad(frame,
    staged): its zero-padding offset (n <= staged) or minus its crop offset (n > staged) — TF's split, odd extra to the
    bottom / right."""
    return (staged - n) // 2 if n <= staged else -((n - staged) // 2)


def pack_desc(shapes, batch, staged=None, nmaps=0, u8=False):
    """The device table of unflow_inference_input / _output (include/unflow_hip.h): int32 [batch][8] =
    {h, w, y0, x0, nmaps, u8, 0, 0} per sample.  shapes: the frames' (h, w), at most `batch` of them (the rest of the
    slots: h = 0, unused).  staged None: raw frames at the origin of their staging row; (Hs, Ws): frames as KITTIInput
    delivers them, cropped / padded to (Hs, Ws) (origins as resize_image_with_crop_or_pad)."""
    if len(shapes) > batch:
        raise ValueError("%d frames for a batch of %d" % (len(shapes), batch))
    d = np.zeros((batch, 8), dtype=np.int32)
    for i, (h, w) in enumerate(shapes):
        y0, x0 = (0, 0) if staged is None else (frame_origin(int(h), staged[0]), frame_origin(int(w), staged[1]))
        d[i] = (int(h), int(w), y0, x0, nmaps, int(bool(u8)), 0, 0)
    return d


def sequence_tables(shape, k, batch, carry, u8=False, max_flow=None, track=None, nmaps=0, held=0):
    """The device tables of one sequence replay, one int32 array [16 * batch + 4]: the frame table [batch][8] (pack_desc: the k
    new frames of size `shape` in rows 1 .. k of the engine, slots [0, k)), the pair table [batch][8] (slot i = rows i, i + 1:
    valid when both hold frames of this clip — slot 0 needs a carried frame, slot i >= 1 needs i + 1 <= k), the carry source
    (row of the previous replay's last frame; 0: a clip's first replay, nothing carried) and, behind it, the max_flow of the
    clip's flow colours (unflow_sequence_visual): 0 for None, every pair coloured with its own maximum, else the bit pattern of
    float32 max(max_flow, 1) (flow_util.py:31-32); behind that, the two words of unflow_sequence_track: track = (S, N), the grid
    stride (0 with sparse anchors) and the number of tracks; None: both 0, as in every table without tracks.  nmaps: the maps of
    the staged ground truth of every valid pair (word 4 of its row; 0: none, the pair is not scored).  held: non-zero when the
    truth frames of every valid pair are staged (word 6 of its row; 0: unflow_sequence_interpolate_score skips the pair).  Returns (table, slots of
    the valid pairs in order, the next replay's carry source = k)."""
    batch, k, carry = int(batch), int(k), int(carry)
    if not 1 <= k <= batch:
        raise ValueError("a sequence replay takes 1 to %d new frames, got %d" % (batch, k))
    if not 0 <= carry <= batch:
        raise ValueError("the carry source is a row in [0, %d], got %d" % (batch, carry))
    tab = np.zeros(16 * batch + 4, dtype=np.int32)
    tab[:8 * batch] = pack_desc([shape] * k, batch, u8=u8).reshape(-1)
    valid = [i for i in range(batch) if i + 1 <= k and (i > 0 or carry > 0)]
    pair = np.zeros((batch, 8), dtype=np.int32)
    for i in valid:
        pair[i] = (int(shape[0]), int(shape[1]), 0, 0, int(nmaps), int(bool(u8)), int(held), 0)
    tab[8 * batch:16 * batch] = pair.reshape(-1)
    tab[16 * batch] = carry
    if max_flow is not None:
        tab[16 * batch + 1] = np.array([max(max_flow, 1)], dtype=np.float32).view(np.int32)[0]
    if track is not None:
        S, N = int(track[0]), int(track[1])
        if S < 0 or not 1 <= N < 2 ** 31:
            raise ValueError("tracks: a grid stride >= 1 (0: sparse anchors) and 1 to 2^31 - 1 tracks, got S = %d, N = %d" % (S, N))
        tab[16 * batch + 2], tab[16 * batch + 3] = S, N
    return tab, valid, k


def sequence_replays(num_frames, batch, shape=(1, 1), u8=False):
    """The replays of a clip of num_frames frames pushed `batch` at a time (estimate_sequence's plan): a list of
    (first new frame, k, table, valid pair slots).  Fewer than two frames give no pair: ValueError."""
    if int(num_frames) < 2:
        raise ValueError("a clip needs at least two frames, got %d" % num_frames)
    out, carry = [], 0
    for n0 in range(0, int(num_frames), int(batch)):
        k = min(int(batch), int(num_frames) - n0)
        tab, valid, nxt = sequence_tables(shape, k, batch, carry, u8)
        out.append((n0, k, tab, valid))
        carry = nxt
    return out


def example_stream(batch_iter):
    """Examples of what KITTIInput.input_{train,test}_{2012,2015}() yields, one tuple per example: batches of
    (im1, im2, input_shape[, flow_occ, mask_occ, flow_noc, mask_noc]) or the 2-map form (..., flow_gt, mask)."""
    for batch in batch_iter:
        if len(batch) not in (3, 5, 7):
            raise ValueError("a batch is (im1, im2, input_shape) + 0, 1 or 2 (flow, mask) pairs; got %d arrays" % len(batch))
        arrs = [np.asarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for t in batch]
        for i in range(arrs[0].shape[0]):
            yield tuple(a[i] for a in arrs)


def chunks(it, n):
    buf = []
    for x in it:
        buf.append(x)
        if len(buf) == n:
            yield buf
            buf = []
    if buf:
        yield buf


def output_buffers(B, Hm, Wm, Ncap=0, n_mid=0, ground_truth=False, held_out=False, stabilise=False, denoise=False):
    """The output buffers of a replay, written down once, in the order they are copied back: (the name a slot's pinned copy has
    and `want` asks for, the estimator's attribute of the device buffer, shape, dtype, the estimator flag it needs — None: every
    estimator has it).  Without its flag both attributes are None.  Ncap: the track capacity of a tracking estimator; n_mid: the
    in-between frames per pair of an interpolating one.  ground_truth: also the rows of unflow_sequence_track_score,
    behind the others; their flag, track_gt, needs track and ground_truth both.  held_out: also the rows of
    unflow_sequence_interpolate_score, behind everything else.  stabilise: also the five rows of
    unflow_sequence_stabilise, behind those.  denoise: also the two rows of unflow_sequence_denoise,
    last."""
    scored = ()
    if ground_truth:
        scored = (('track_scores', 'out_track_scores', (B, 16), torch.int32, 'track_gt'),
                  ('track_err', 'out_track_err', (B,), torch.float64, 'track_gt'),
                  ('gt_track_disp', 'out_gt_track_disp', (B, Ncap, 2), torch.float32, 'track_gt'),
                  ('gt_track_alive', 'out_gt_track_alive', (B, Ncap), torch.uint8, 'track_gt'))
    if held_out:
        scored += (('mid_sse', 'out_mid_sse', (n_mid, B, 3), torch.int64, 'held_out'),
                   ('mid_ssim', 'out_mid_ssim', (n_mid, B, 3), torch.float64, 'held_out'))
    if stabilise:
        scored += (('stab', 'out_stab', (B, Hm, Wm, 3), torch.uint8, 'stabilise'),
                   ('stab_resid', 'out_stab_resid', (B, Hm, Wm), torch.uint8, 'stabilise'),
                   ('stab_motion', 'out_stab_motion', (B, 8), torch.int64, 'stabilise'),
                   ('stab_path', 'out_stab_path', (B, 8), torch.int64, 'stabilise'),
                   ('stab_counts', 'out_stab_counts', (B, 4), torch.int32, 'stabilise'))
    if denoise:
        scored += (('den', 'out_den', (B, Hm, Wm, 3), torch.uint8, 'denoise'),
                   ('den_stats', 'out_den_stats', (B, 8), torch.int32, 'denoise'))
    return (('flow', 'out_flow', (B, Hm, Wm, 2), torch.float32, None),
            ('u16', 'out_u16', (B, Hm, Wm, 3), torch.int16, None),
            ('sums', 'sums', (B, 2, 2), torch.float64, None),
            ('counts', 'counts', (B, 2), torch.int32, None),
            ('flow_bw', 'out_flow_bw', (B, Hm, Wm, 2), torch.float32, 'bidirectional'),
            ('u16_bw', 'out_u16_bw', (B, Hm, Wm, 3), torch.int16, 'bidirectional'),
            ('occ', 'occ', (2, B, Hm, Wm), torch.uint8, 'bidirectional'),                   # occ_fw, occ_bw
            ('occ_counts', 'occ_counts', (B, 3), torch.int32, 'bidirectional'),
            ('vis', 'vis', (len(VISUAL_IMAGES), B, Hm, Wm, 3), torch.uint8, 'visual'),
            ('track_disp', 'out_track_disp', (B, Ncap, 2), torch.float32, 'track'),
            ('track_alive', 'out_track_alive', (B, Ncap), torch.uint8, 'track'),
            ('mid', 'out_mid', (n_mid, B, Hm, Wm, 3), torch.uint8, 'interpolate'),
            ('mid_holes', 'out_mid_holes', (n_mid, B), torch.int32, 'interpolate')) + scored


class _Slot:
    """One set of pinned host buffers and the event of the last device work that read or wrote them."""

    def __init__(self, est):
        B, Hm, Wm = est.B, est.Hmax, est.Wmax
        pin = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, pin_memory=True)   # noqa: E731
        nfr = 1 if est.sequence else 2                                       # sequence: B new frames per replay, not 2B
        self.frames = pin(nfr * B * Hm * Wm * 3 * 4, dtype=torch.uint8)      # fp32-sized; uint8 frames use the first quarter
        self.desc = pin(B, 8, dtype=torch.int32)
        self.tab = pin(16 * B + 4, dtype=torch.int32) if est.sequence else None   # sequence_tables
        self.gt_flow = self.gt_mask = None
        # held_out: the truth frames of a replay's pairs, [n_mid][B][Hmax][Wmax][3], fp32-sized like the frames
        self.truth = pin(est.interpolate * B * Hm * Wm * 3 * 4, dtype=torch.uint8) if est.held_out else None
        for name, _, shape, dtype, flag in output_buffers(B, Hm, Wm, est.track_cap, est.interpolate, True, held_out=True,
                                                          stabilise=True, denoise=True):
            setattr(self, name, pin(*shape, dtype=dtype) if flag is None or getattr(est, flag) else None)
        self.event = None
        self.pending = None      # the rows of the last replay as ([(slot row i, h, w), ...], nmaps): set by FlowEstimator._replay
        self.scan = self.scan_table = self.spans = None      # files through the device encode path (FlowEstimator._encoder)
        self.scan_kind = 'png'                               # what slot.scan holds per span: scanlines, or 'png_z' zlib streams

    def scan_buffers(self, enc):
        """The pinned scanline buffer and table of this slot, sized like the estimator's device ones."""
        if self.scan is None:
            self.scan = torch.zeros(enc.host_bytes, dtype=torch.uint8, pin_memory=True)
            self.scan_table = torch.zeros(tuple(enc.table.shape), dtype=torch.int64, pin_memory=True)
        return self.scan, self.scan_table

    def gt(self, est):
        if self.gt_flow is None:
            B, Hm, Wm = est.B, est.Hmax, est.Wmax
            self.gt_flow = torch.zeros(2, B, Hm, Wm, 2, pin_memory=True)
            self.gt_mask = torch.zeros(2, B, Hm, Wm, pin_memory=True)
        return self.gt_flow, self.gt_mask

    def wait(self):
        if self.event is not None:
            self.event.synchronize()


class _Encoder:
    """The device half of FlowEstimator's file output (csrc/png_encode.hip): the surfaces unflow_png_filter reads — the
    estimator's own output buffers, no staging copy — a device table and the device scanline buffer, sized for every file one
    replay can ask for.  deflater: the buffers of unflow_deflate (png_device.DeviceDeflater), allocated with the first
    deflate='device' call; host_bytes: what a slot's pinned buffer holds at the most — the scanlines, or their zlib streams
    at the stream bound."""

    def __init__(self, est):
        from .png_device import PngSurface
        B, Hm, Wm = est.B, est.Hmax, est.Wmax
        named = [('u16', est.out_u16, B, 3, _lib.PNG_U16BE)]
        if est.bidirectional:
            named += [('u16_bw', est.out_u16_bw, B, 3, _lib.PNG_U16BE), ('occ', est.occ[0], B, 1, _lib.PNG_U8X255)]
        if est.visual:
            named += [('vis', est.vis, len(VISUAL_IMAGES) * B, 3, _lib.PNG_U8)]
        if est.interpolate:
            named += [('mid', est.out_mid, est.interpolate * B, 3, _lib.PNG_U8)]
        if est.stabilise:
            named += [('stab', est.out_stab, B, 3, _lib.PNG_U8), ('stab_resid', est.out_stab_resid, B, 1, _lib.PNG_U8)]
        if est.denoise:
            named += [('den', est.out_den, B, 3, _lib.PNG_U8)]
        self.index = {name: k for k, (name, *_) in enumerate(named)}
        self.surfaces = [PngSurface(t, images, Hm, Wm, ch, kind) for _, t, images, ch, kind in named]
        n_files = sum(s.images for s in self.surfaces)
        n_bytes = sum(s.images * Hm * (1 + Wm * s.bpp) for s in self.surfaces)
        self.n_files, self.deflater = n_files, None
        self.host_bytes = n_bytes + 5 * (n_bytes // _lib.DEFLATE_CHUNK_DEFAULT + n_files) + 6 * n_files
        with torch.cuda.device(est.dev):
            self.table = torch.zeros(n_files, _lib.PNG_FILTER_FIELDS, dtype=torch.int64, device=est.dev)
            self.scan = torch.zeros(n_bytes, dtype=torch.uint8, device=est.dev)


class FlowEstimator:
    """Frame-size optical flow of a trained FlowNet spec (params['flownet'], 'full_res', ...), `batch` pairs per replay at the
    network size net_size = (H, W) (divisible by 64), frames of any size up to max_frame (default: net_size).
    bidirectional: also the backward flow and the forward-backward occlusion masks (estimate_bidirectional, the occlusion
    scores of evaluate, export's backward / occlusion files).  visual: also the 8-bit pictures of every batch (visualize,
    export(visual=True)).
    sequence: the estimator of a clip — reset / push / estimate_sequence / export_sequence: the flow from every frame to the
    next, each frame uploaded and encoded once; the pair methods (estimate, evaluate, export, ...) then raise RuntimeError, as
    the sequence methods do on a pair estimator.  sequence='bidirectional': the same along a clip in both directions —
    push_bidirectional / estimate_sequence_bidirectional give the backward flow and both occlusion masks of every pair,
    export_sequence its backward / occlusion files; push and estimate_sequence still return the forward flows alone.  (Not
    spelt bidirectional=True with sequence: ValueError.)  With visual='sequence' (visual=True with sequence: ValueError, as
    before; the message names this spelling): the pictures of every pair of the clip, every frame
    resampled once (push_visual, visualize_sequence, export_sequence(visual=True)): FlowVisual per pair, or SequenceVisual on a
    sequence='bidirectional' estimator; max_flow there is one scale of the flow colours for the whole clip, set by the call that
    starts the clip (None: every pair has its own maximum, as in pair mode).
    track (with sequence): tracks along a clip — where the pixels of the clip's first frame are in every later frame, the forward
    flows chained through image_warp's taps, and whether each is still visible (inside the frame; on a sequence='bidirectional'
    estimator also: never under the forward occlusion mask).  True: an anchor at every pixel; an int S >= 1: at every S-th pixel
    of every S-th row; an int array [N][2]: at those (x, y).  push_tracks / track_sequence return a Track(disp, alive) per pair,
    export_sequence(tracks=True) writes them; every other method returns what it returns without track.  reset() starts a new
    anchor frame.
    interpolate (with sequence): n in 1..7 in-between frames per pair of the clip, motion-compensated on the device from the
    staged frames and the flows (both directions and the occlusion masks on a sequence='bidirectional' estimator).
    push_interpolated / interpolate_sequence return an Interpolated(frames, holes) per pair, export_sequence(interpolate=True)
    writes them; every other method returns what it returns without interpolate.  reset() starts a new clip: the frame kept
    from the last one is not used.
    interpolate_order (with interpolate): k in 1..4, the consistency-ordered splat — every splatted pixel is weighted
    by how well the two frames agree along its flow (the weight halves per 64 >> k summed grey levels), pixels that disagree are
    not blended, and on a one-direction estimator a hole takes the later frame's colour.  None or 0: the plain splat.  Nothing
    else changes: the same methods, tuples and files.
    ground_truth (with sequence): the pairs of a clip are scored against ground truth given with the frames — push_scored returns
    a PairScore per pair (AEE and outliers per map; the occlusion counts with both directions and two maps; with track a
    TrackScore against the chained ground-truth flow), evaluate_sequence the averages over clips; every other method returns
    what it returns without ground_truth.
    held_out (with interpolate): the in-between frames are scored against the frames that were left out of the clip, given with
    the frames — push_held_out returns a HeldOut(frames, holes, sse, psnr, ssim) per pair, for the interpolated frame, the temporal
    blend and the nearest frame; evaluate_interpolation subsamples full-rate clips and pools the scores; every other method
    returns what it returns without held_out.
    stabilise (with sequence): True or dict(tol=2, iters=3, follow=0) — the camera motion of the clip: per pair a
    robust affine fit to the forward flow (tol in 0..4: a pixel's weight halves per 2^(1 - tol) px of residual; iters in 0..4
    reweighted fits behind the first), the pixels that do not follow it, and the later frame resampled along the composed camera
    path (follow = 0: locked on the clip's first frame; s in 1..8: the path loses 2^-s of its offset per pair).  push_stabilised /
    stabilise_sequence return a Stabilised(frame, residual, motion, path, counts) per pair, export_sequence(stabilise=True) writes
    them; every other method returns what it returns without stabilise.  reset() starts a new path.
    denoise (with sequence='bidirectional'): True or dict(tol='auto', depth=8) — temporal noise reduction: every
    frame of the clip is averaged with its own history, fetched along the backward flow; a pixel without a usable source (no
    valid flow, a source outside the frame, occluded) starts a new history, one whose history is too far from the frame drops
    it (tol in 0..4: the distance that halves the history's weight is 8 * 2^tol grey levels; 'auto': chosen per pair from its
    noise level), and depth in 1..64 bounds the length of the average.  push_denoised / denoise_sequence return a
    Denoised(frame, noise, tol, counts) per pair, export_sequence(denoise=True) writes the frames; every other method returns what
    it returns without denoise.  reset() starts a new history."""

    def __init__(self, params, batch, net_size=(384, 1280), max_frame=None, device=None, use_graph=True, bidirectional=False,
                 visual=False, sequence=False, track=False, interpolate=None, ground_truth=False, held_out=False,
                 interpolate_order=None, stabilise=None, denoise=None):
        if not isinstance(sequence, bool) and sequence != 'bidirectional':
            raise ValueError("FlowEstimator: sequence is False, True or 'bidirectional', got %r" % (sequence,))
        if sequence and bidirectional:
            raise ValueError("FlowEstimator: both directions along a clip are sequence='bidirectional', not bidirectional=True "
                             "with sequence")
        if not isinstance(visual, bool) and visual != 'sequence':
            raise ValueError("FlowEstimator: visual is False, True or 'sequence', got %r" % (visual,))
        if sequence and visual is True:
            raise ValueError("FlowEstimator: the pictures along a clip are visual='sequence' (a shown frame per engine row, "
                             "unflow_sequence_visual), not visual=True with sequence")
        if visual == 'sequence' and not sequence:
            raise ValueError("FlowEstimator: visual='sequence' draws the pairs of a clip; it needs sequence=True or "
                             "sequence='bidirectional' (a pair estimator's pictures are visual=True)")
        self.track_spec = track_option(track)
        if self.track_spec is not None and not sequence:
            raise ValueError("FlowEstimator: track follows the pixels of a clip's first frame; it needs sequence=True or "
                             "sequence='bidirectional'")
        self.track = self.track_spec is not None
        self.interpolate = interpolate_option(interpolate)       # in-between frames per pair; 0: none
        if self.interpolate and not sequence:
            raise ValueError("FlowEstimator: interpolate makes the frames between the frames of a clip; it needs sequence=True or "
                             "sequence='bidirectional'")
        self.interpolate_order = interpolate_order_option(interpolate_order, self.interpolate)    # 0: the plain splat
        self.held_out = bool(held_out)                           # the in-between frames are scored
        if self.held_out and not self.interpolate:
            raise ValueError("FlowEstimator: held_out scores the in-between frames against the frames left out of the clip; it "
                             "needs interpolate=n (and sequence=True or sequence='bidirectional')")
        self.stabilise = stabilise_option(stabilise)             # camera motion along the clip; None: none
        if self.stabilise and not sequence:
            raise ValueError("FlowEstimator: stabilise fits the camera motion along a clip; it needs sequence=True or "
                             "sequence='bidirectional'")
        self.denoise = denoise_option(denoise)                   # temporal denoising along the clip; None: none
        if self.denoise and sequence != 'bidirectional':
            raise ValueError("FlowEstimator: denoise averages a frame with its history, which is fetched along the backward flow "
                             "and dropped under the backward occlusion mask; it needs sequence='bidirectional' (got sequence=%r)"
                             % (sequence,))
        self.ground_truth = bool(ground_truth)                   # sequence: the clip's pairs are scored
        if self.ground_truth and not sequence:
            raise ValueError("FlowEstimator: ground_truth scores the pairs of a clip; it needs sequence=True or "
                             "sequence='bidirectional' (a pair estimator scores already: evaluate)")
        self.track_gt = self.track and self.ground_truth
        self.sequence = bool(sequence)
        self.seq_bidir = sequence == 'bidirectional'
        self.params = dict(params)
        self.B = int(batch)
        self.H, self.W = (int(v) for v in net_size)
        self.Hmax, self.Wmax = (int(v) for v in (max_frame or net_size))
        self.dev = torch.device('cuda:0') if device is None else torch.device(device)
        self.use_graph = bool(use_graph)
        self.bidirectional = bool(bidirectional) or self.seq_bidir
        self.visual = bool(visual)
        # track capacity: the dense grid over max_frame, or the anchors given
        self.track_cap = 0
        if self.track:
            kind, arg = self.track_spec
            self.track_cap = int(np.prod(track_grid((self.Hmax, self.Wmax), arg))) if kind == 'dense' else int(arg.shape[0])
        eng_params = {k: v for k, v in self.params.items() if k.endswith('_weight') or k in ENGINE_KEYS}
        self.engine = FlowNetEngine(self.B, self.H, self.W, params=eng_params or None, device=self.dev, seed=None,
                                    inference=True, bidirectional=bool(bidirectional), sequence=sequence)
        e = self.engine
        B, Hm, Wm = self.B, self.Hmax, self.Wmax
        L = _lib.lib()
        with torch.cuda.device(self.dev):
            z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.dev)   # noqa: E731
            self.frames = z((1 if self.sequence else 2) * B * Hm * Wm * 3 * 4, dtype=torch.uint8)
            self.desc = z(B, 8, dtype=torch.int32)
            # sequence: frame table, pair table and carry source in one buffer (sequence_tables); ground truth only on request
            self.tab = z(16 * B + 4, dtype=torch.int32) if self.sequence else None
            scored = self.ground_truth or not self.sequence
            self.gt_flow, self.gt_mask = (z(2, B, Hm, Wm, 2), z(2, B, Hm, Wm)) if scored else (None, None)
            nb = int(L.unflow_inference_output_blocks(Hm, Wm))
            self.partial = z(B * nb * 6, dtype=torch.float64)
            self.ticket = z(B, dtype=torch.int32)
            for _, attr, shape, dtype, flag in output_buffers(B, Hm, Wm, self.track_cap, self.interpolate, True,
                                                              held_out=True, stabilise=True, denoise=True):     # out_flow, ...
                setattr(self, attr, z(*shape, dtype=dtype) if flag is None or getattr(self, flag) else None)
            self.track_anchors = self.track_disp = self.track_alive = None
            if self.track:
                # the state of unflow_sequence_track, kept from one replay of a clip to the next; sparse: the anchor table
                self.track_disp, self.track_alive = z(self.track_cap, 2), z(self.track_cap, dtype=torch.uint8)
                if self.track_spec[0] == 'sparse':
                    self.track_anchors = torch.from_numpy(self.track_spec[1]).to(self.dev)
            self.gt_track_disp = self.gt_track_alive = self.track_score_ws = None
            if self.track_gt:
                # the state of unflow_sequence_track_score, kept along a clip like the tracks', and its scratch: zero now and
                # left zero by every launch
                self.gt_track_disp, self.gt_track_alive = z(self.track_cap, 2), z(self.track_cap, dtype=torch.uint8)
                self.track_score_ws = z(int(L.unflow_sequence_track_score_workspace_bytes(B, self.track_cap)) // 8,
                                        dtype=torch.int64)
            self.mid_prev = self.mid_sums = None
            if self.interpolate:
                # unflow_sequence_interpolate: the clip's last staged frame, kept from one replay to the next (fp32-sized), and the
                # 64-bit sums, zero now and left zero by every launch
                self.mid_prev = z(Hm * Wm * 3 * 4, dtype=torch.uint8)
                self.mid_sums = z(int(L.unflow_sequence_interpolate_workspace_bytes(self.interpolate, B, Hm, Wm)) // 8,
                                  dtype=torch.int64)
            self.mid_truth = self.mid_score_prev = self.mid_score_ws = None
            if self.held_out:
                # unflow_sequence_interpolate_score: the staged truth frames (fp32-sized), its own copy of the clip's last frame and
                # its scratch, zero now and left zero by every launch
                self.mid_truth = z(self.interpolate * B * Hm * Wm * 3 * 4, dtype=torch.uint8)
                self.mid_score_prev = z(Hm * Wm * 3 * 4, dtype=torch.uint8)
                self.mid_score_ws = z(int(L.unflow_sequence_interpolate_score_workspace_bytes(self.interpolate, B, Hm, Wm)) // 8,
                                      dtype=torch.int64)
            self.stab_path = self.stab_identity = self.stab_ws = None
            if self.stabilise:
                # unflow_sequence_stabilise: the camera path, kept from one replay of a clip to the next (never read while the
                # carry source is 0: reset() needs no memset), and its workspace, zero now and left zero by every launch
                self.stab_path = z(8, dtype=torch.int64)
                self.stab_identity = torch.tensor([0, 1 << 24, 0, 0, 0, 1 << 24, 0, 0], dtype=torch.int64, device=self.dev)
                self.stab_ws = z(int(L.unflow_sequence_stabilise_workspace_bytes(B)) // 8, dtype=torch.int64)
            self.den_state = self.den_ws = None
            if self.denoise:
                # unflow_sequence_denoise: the history (an 8.8 colour and a count per pixel), kept from one replay of a clip to the
                # next (re-initialised on the device while the carry source is 0: reset() needs no memset), and its workspace —
                # the histograms, zero now and left zero by every launch, then the two history slabs
                self.den_state = z(Hm, Wm, 4, dtype=torch.int16)
                self.den_ws = z(int(L.unflow_sequence_denoise_workspace_bytes(B, Hm, Wm)) // 4, dtype=torch.int32)
            self.vis_shown = self.vis_max = None
            if self.visual:
                # the frames as shown: resized to the network and back; sequence: one per engine row, row 0 carried
                self.vis_shown = z(B + 1, Hm, Wm, 4) if self.sequence else z(2, B, Hm, Wm, 4)
                self.vis_max = z(3 * B, dtype=torch.int32)           # bit patterns of max |flow|, max |gt * mask|; B tickets
        last = e.stages[-1]
        self.flow_src = last.act['flow0'] if e.full_res else last.act['flow2']     # bidirectional: rows [0, B) fw, [B, 2B) bw
        self.in_planes = e.network_input_planes()
        self.slots = None
        self.graph = None
        self.global_step = None
        self._dims = None             # the staged (KITTIInput) frame size of the current evaluate / export pass
        self._carry = 0               # sequence: the row that holds the clip's last frame (0: none yet)
        self._clip = None             # sequence: (h, w, dtype is uint8) of the clip's frames
        self._seq_k = 0               # sequence: replays submitted (the pinned slot alternates)
        self._max_flow = _UNSET       # sequence: the clip's max_flow of the flow colours (None: per pair), set by its first push
        self._enc = None              # _Encoder, built by the first export through the device encode path
        self._clip_nmaps = 0          # sequence with ground_truth: the maps per pair of the clip, set by its first scored pair

    # ------------------------------------------------------------------------------------------ parameters
    @classmethod
    def from_checkpoint(cls, ckpt_dir, params, *args, **kwargs):
        """An estimator with the networks Trainer.restore(ckpt_dir, engine=...) would restore: the trained networks from the
        latest checkpoint of ckpt_dir, frozen networks of a stack from params['finetune'] (or the checkpoint, when it holds
        them).  A network with no source is an error (train.network_files(strict=True))."""
        from .input import restore_networks
        from .train import network_files
        est = cls(params, *args, **kwargs)
        files, ckpt = network_files(est.params, est.engine.spec, ckpt_dir, strict=True)
        restore_networks(est.engine, est.params, files)
        est._params_changed()
        est.global_step = None if ckpt is None else int(os.path.basename(ckpt).split('-')[-1])
        return est

    def load_tf_params(self, tf_params):
        self.engine.load_tf_params(tf_params)
        self._params_changed()

    def _params_changed(self):
        with torch.cuda.device(self.dev):
            self.engine.refresh_weight_planes(force=True)      # the captured graph does not re-split: weights are static here

    # ------------------------------------------------------------------------------------------ device work
    def _launch(self):
        """Input kernel, forward pass, output kernel on the current stream (what the graph holds); bidirectional: then the
        output kernel on the backward rows and the occlusion kernel; visual: then the pictures."""
        e = self.engine
        L = _lib.lib()
        st = e.stream()
        if self.sequence:
            return self._launch_sequence()
        check(L.unflow_inference_input(ptr(self.frames), ptr(self.desc), self.B, self.Hmax, self.Wmax, self.H, self.W,
                                       ptr(e.x0), e.mean_host, _lib.planes_of(self.in_planes), st), "inference_input")
        e.forward_net()
        self._output(self.flow_src, self.desc, self.out_flow, self.out_u16, gt=True)
        if self.bidirectional:
            self._launch_backward()
        if self.visual:
            check(L.unflow_inference_visual(ptr(self.frames), ptr(self.desc), self.B, self.Hmax, self.Wmax, self.H, self.W,
                                            ptr(self.out_flow), ptr(self.gt_flow), ptr(self.gt_mask), ptr(self.vis_shown),
                                            ptr(self.vis_max), ptr(self.vis), None, st), "inference_visual")

    def _launch_sequence(self):
        """Carry, input of the new frames, forward pass, output kernel over the pair table (what the sequence graph holds);
        sequence='bidirectional': the output kernel on either block of the engine's 2B rows, then the occlusion kernel, all
        three over the pair table and without ground truth (denoise: then the denoised frames); track: then the tracks, through the pairs of the table; interpolate:
        then the in-between frames of those pairs (held_out: and their scores where the table says held); visual: then the pictures, from the same tables."""
        e, B = self.engine, self.B
        L = _lib.lib()
        e.sequence_carry(self.tab[16 * B:])
        e.sequence_input(self.frames, self.tab, self.Hmax, self.Wmax)
        e.forward_net()
        pairs = self.tab[8 * B:]
        if self.seq_bidir:
            fw, bw = e.fw_bw(self.flow_src)
            self._output(fw, pairs, self.out_flow, self.out_u16, gt=self.ground_truth)
            self._output(bw, pairs, self.out_flow_bw, self.out_u16_bw)
            self._occlusion(pairs, self.gt_mask if self.ground_truth else None)
            if self.denoise:
                o = self.denoise
                check(L.unflow_sequence_denoise(ptr(self.frames), ptr(self.tab), B, self.Hmax, self.Wmax, ptr(self.out_flow_bw),
                                                ptr(self.occ[1]), -1 if o['tol'] == 'auto' else o['tol'], o['depth'],
                                                ptr(self.den_state), ptr(self.den_ws), ptr(self.out_den), ptr(self.out_den_stats),
                                                e.stream()), "sequence_denoise")
        else:
            self._output(self.flow_src, pairs, self.out_flow, self.out_u16, gt=self.ground_truth)
        if self.track:
            check(L.unflow_sequence_track(ptr(self.out_flow), ptr(self.occ[0]) if self.seq_bidir else None, ptr(self.tab), B,
                                          self.Hmax, self.Wmax, ptr(self.track_anchors), self.track_cap, ptr(self.track_disp),
                                          ptr(self.track_alive), ptr(self.out_track_disp), ptr(self.out_track_alive),
                                          e.stream()), "sequence_track")
        if self.track_gt:
            check(L.unflow_sequence_track_score(ptr(self.gt_flow), ptr(self.gt_mask), ptr(self.tab), B, self.Hmax, self.Wmax,
                                                ptr(self.track_anchors), self.track_cap, ptr(self.out_track_disp),
                                                ptr(self.out_track_alive), ptr(self.gt_track_disp), ptr(self.gt_track_alive),
                                                ptr(self.out_gt_track_disp), ptr(self.out_gt_track_alive),
                                                ptr(self.out_track_scores), ptr(self.out_track_err), ptr(self.track_score_ws),
                                                e.stream()), "sequence_track_score")
        if self.stabilise:
            o = self.stabilise
            check(L.unflow_sequence_stabilise(ptr(self.frames), ptr(self.tab), B, self.Hmax, self.Wmax, ptr(self.out_flow),
                                              ptr(self.occ[0]) if self.seq_bidir else None, o['tol'], o['iters'], o['follow'],
                                              ptr(self.stab_path), ptr(self.stab_ws), ptr(self.out_stab_motion),
                                              ptr(self.out_stab_path), ptr(self.out_stab_resid), ptr(self.out_stab),
                                              ptr(self.out_stab_counts), e.stream()), "sequence_stabilise")
        if self.interpolate:
            bw, ofw, obw = (self.out_flow_bw, self.occ[0], self.occ[1]) if self.seq_bidir else (None, None, None)
            args = (ptr(self.frames), ptr(self.tab), B, self.Hmax, self.Wmax, self.interpolate, ptr(self.out_flow), ptr(bw), ptr(ofw),
                    ptr(obw), ptr(self.mid_prev), ptr(self.mid_sums), ptr(self.out_mid), ptr(self.out_mid_holes))
            if self.interpolate_order:
                check(L.unflow_sequence_interpolate_ordered(*args, self.interpolate_order, e.stream()), "sequence_interpolate_ordered")
            else:
                check(L.unflow_sequence_interpolate(*args, e.stream()), "sequence_interpolate")
        if self.held_out:
            check(L.unflow_sequence_interpolate_score(ptr(self.frames), ptr(self.tab), B, self.Hmax, self.Wmax, self.interpolate,
                                                      ptr(self.out_mid), ptr(self.mid_truth), ptr(self.mid_score_prev),
                                                      ptr(self.mid_score_ws), ptr(self.out_mid_sse), ptr(self.out_mid_ssim),
                                                      e.stream()), "sequence_interpolate_score")
        if self.visual:
            bw, occ = (self.out_flow_bw, self.occ[0]) if self.seq_bidir else (None, None)
            check(L.unflow_sequence_visual(ptr(self.frames), ptr(self.tab), B, self.Hmax, self.Wmax, self.H, self.W,
                                           ptr(self.out_flow), ptr(bw), ptr(occ), ptr(self.vis_shown), ptr(self.vis_max),
                                           ptr(self.vis), None, e.stream()), "sequence_visual")

    def _launch_backward(self):
        self._output(self.flow_src[self.B:], self.desc, self.out_flow_bw, self.out_u16_bw, what="inference_output (backward)")
        self._occlusion(self.desc, self.gt_mask)

    def _output(self, src, table, flow, u16, gt=False, what="inference_output"):
        """unflow_inference_output on rows `src` of the engine's flow, driven by `table` (the descriptor table or the pair
        table): the frame-size flow and its 16-bit encoding.  gt: also scored against the staged ground truth (sums, counts);
        only the forward rows of a pair estimator are."""
        f = self.flow_src
        scoring = [None] * 6
        if gt:
            scoring = [ptr(t) for t in (self.gt_flow, self.gt_mask, self.partial, self.ticket, self.sums, self.counts)]
        check(_lib.lib().unflow_inference_output(ptr(src), f.shape[1], f.shape[2], _lib.cf(FLOW_SCALE * 4), self.H, self.W,
                                                 ptr(table), self.B, self.Hmax, self.Wmax, ptr(flow), ptr(u16), *scoring,
                                                 self.engine.stream()), what)

    def _occlusion(self, table, gt_mask=None):
        """unflow_inference_occlusion on the two frame-size flows: both masks; with KITTI's mask (pair mode), the counts."""
        check(_lib.lib().unflow_inference_occlusion(ptr(self.out_flow), ptr(self.out_flow_bw), ptr(table), self.B, self.Hmax,
                                                    self.Wmax, None if gt_mask is None else ptr(gt_mask), ptr(self.occ[0]),
                                                    ptr(self.occ[1]), ptr(self.occ_counts), self.engine.stream()),
              "inference_occlusion")

    def _run(self):
        e = self.engine
        if not self.use_graph:
            self._launch()
            return
        if self.graph is None:
            e.refresh_weight_planes(force=True)
            e.planes_external = True          # the weights are static: the graph does not re-split them
            self._launch()                    # eager pass first: grows the shared workspaces outside the capture
            # (sequence: the eager pass and the first replay both run the carry; the graph is built by an estimator's first
            # replay ever, whose carry source is 0 — a no-op both times; unflow_sequence_track starts from disp = 0, alive = 1
            # both times for the same reason)
            torch.cuda.current_stream(self.dev).synchronize()
            s = torch.cuda.Stream(self.dev)
            s.wait_stream(torch.cuda.current_stream(self.dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    self._launch()
            torch.cuda.current_stream(self.dev).wait_stream(s)
            self.graph = g
        self.graph.replay()

    def _filter(self, slot, entries, deflate=False):
        """The files of one replay through the device encode path: entries [(surface name, image, h, w), ...] -> one
        unflow_png_filter launch on the current stream, right behind the replay and OUTSIDE the captured graph (the set of
        wanted files varies per call), and the copy of the scanlines into the slot's pinned buffer.  slot.spans: per entry
        (offset, bytes, h, w, depth, colour type) in that buffer.
        deflate: the unflow_deflate launches follow the filter launch on the same stream and the pinned buffer
        receives the zlib streams instead (slot.scan_kind 'png_z'; a span's bytes are the stream's).  Their sizes are known only
        behind the kernels, so this waits for the replay once — the writer pool, not this thread, sets an export's pace — and
        then queues one copy per stream of exactly its bytes."""
        from .png_device import DeviceDeflater, filter_scanlines, plan_scanlines
        slot.scan_kind = 'png_z' if deflate else 'png'
        if not entries:
            slot.spans = []
            return
        if self._enc is None:
            self._enc = _Encoder(self)
        enc = self._enc
        scan, table = slot.scan_buffers(enc)
        rows, spans, total, max_h, max_row = plan_scanlines(enc.surfaces, [(enc.index[s], im, h, w) for s, im, h, w in entries])
        slot.spans = spans
        n = len(entries)
        table.numpy()[:n] = rows
        enc.table[:n].copy_(table[:n], non_blocking=True)
        cur = torch.cuda.current_stream(self.dev)
        filter_scanlines(enc.surfaces, enc.table, n, max_h, max_row, enc.scan, cur)
        if not deflate:
            scan[:total].copy_(enc.scan[:total], non_blocking=True)
            return
        if enc.deflater is None:
            enc.deflater = DeviceDeflater(self.dev, enc.n_files, enc.scan.numel())
        plan = enc.deflater.launch(enc.scan, spans, cur)
        cur.synchronize()
        places = enc.deflater.fetch(plan, scan, cur)
        slot.spans = [(o, nb) + sp[2:] for (o, nb), sp in zip(places, spans)]

    # ------------------------------------------------------------------------------------------ staging
    def _slot(self, k):
        if self.slots is None:
            self.slots = [_Slot(self), _Slot(self)]
        return self.slots[k % 2]

    def _stage(self, slot, examples, staged, nmaps):
        """Pack up to B examples (im1, im2, (h, w)[, gt flow, mask ...]) into the pinned slot; returns (desc, frame bytes)."""
        B, Hm, Wm = self.B, self.Hmax, self.Wmax
        u8 = all(np.asarray(ex[0]).dtype == np.uint8 and np.asarray(ex[1]).dtype == np.uint8 for ex in examples)
        esz = 1 if u8 else 4
        nbytes = 2 * B * Hm * Wm * 3 * esz
        fr = slot.frames[:nbytes].numpy().view(np.uint8 if u8 else np.float32).reshape(2, B, Hm, Wm, 3)
        shapes = []
        for i, ex in enumerate(examples):
            h, w = int(ex[2][0]), int(ex[2][1])
            if h > Hm or w > Wm:
                raise ValueError("a %dx%d frame exceeds max_frame %dx%d" % (h, w, Hm, Wm))
            shapes.append((h, w))
            for k in range(2):
                a = np.asarray(ex[k])
                hs, ws = a.shape[:2]
                if hs > Hm or ws > Wm:
                    raise ValueError("a staged frame of %dx%d exceeds max_frame %dx%d" % (hs, ws, Hm, Wm))
                fr[k, i, :hs, :ws] = a
                if staged is not None:           # the parts of the row outside the staged array read as zero
                    fr[k, i, hs:] = 0
                    fr[k, i, :hs, ws:] = 0
            if nmaps:
                gf, gm = slot.gt(self)
                for m in range(nmaps):
                    f, msk = np.asarray(ex[3 + 2 * m], dtype=np.float32), np.asarray(ex[4 + 2 * m], dtype=np.float32)
                    hs, ws = f.shape[:2]
                    gfa, gma = gf[m, i].numpy(), gm[m, i].numpy()
                    gfa[:hs, :ws] = f
                    gma[:hs, :ws] = msk.reshape(hs, ws)
                    gfa[hs:] = 0
                    gfa[:hs, ws:] = 0
                    gma[hs:] = 0
                    gma[:hs, ws:] = 0
        slot.desc.numpy()[:] = pack_desc(shapes, B, staged, nmaps, u8)
        return shapes, nbytes

    def _stage_device(self, slot, batch, n, staged, nmaps):
        """_stage for the first n examples of a batch whose tensors are already on this device (core/png_device.py's
        iterators): the same descriptor table, and device-to-device copies on the current stream into the fp32 layout of
        self.frames, self.gt_flow and self.gt_mask with the same zeroing outside the staged region — the buffers the host
        path would have uploaded.  Returns the frames' shapes."""
        B, Hm, Wm = self.B, self.Hmax, self.Wmax
        hs, ws = staged
        if hs > Hm or ws > Wm:
            raise ValueError("a staged frame of %dx%d exceeds max_frame %dx%d" % (hs, ws, Hm, Wm))
        if isinstance(batch[2], torch.Tensor) and batch[2].device.type != 'cpu':
            raise ValueError("input_shape of a device batch must stay on the host (reading it would wait for the device)")
        shp = np.asarray(batch[2])
        shapes = [(int(shp[i][0]), int(shp[i][1])) for i in range(n)]
        for h, w in shapes:
            if h > Hm or w > Wm:
                raise ValueError("a %dx%d frame exceeds max_frame %dx%d" % (h, w, Hm, Wm))
        slot.desc.numpy()[:] = pack_desc(shapes, B, staged, nmaps, False)

        def put(dst, src):                   # dst [n, Hm, Wm(, c)] <- src [n, hs, ws(, c)]; zero outside
            dst[:, :hs, :ws].copy_(src, non_blocking=True)
            if hs < Hm:
                dst[:, hs:].zero_()
            if ws < Wm:
                dst[:, :hs, ws:].zero_()
        with torch.cuda.device(self.dev):
            self.desc.copy_(slot.desc, non_blocking=True)
            fr = self.frames.view(torch.float32).view(2, B, Hm, Wm, 3)
            for k in range(2):
                put(fr[k, :n], batch[k][:n])
            for m in range(nmaps):
                put(self.gt_flow[m, :n], batch[3 + 2 * m][:n])
                put(self.gt_mask[m, :n], batch[4 + 2 * m][:n].reshape(n, hs, ws))
        return shapes

    def _submit(self, k, examples, staged=None, nmaps=0, want=('flow',), device_batch=None, files=None):
        """Stage batch k into its slot, copy it in, run, and queue the copies back; returns the slot.  device_batch: (batch,
        n) — the first n examples of a batch of device tensors instead of `examples`.  want, files: _replay's."""
        slot = self._slot(k)
        slot.wait()                               # the last replay that read this slot's buffers (and its copies back) is done
        if device_batch is not None:
            shapes = self._stage_device(slot, device_batch[0], device_batch[1], staged, nmaps)
        else:
            shapes, nbytes = self._stage(slot, examples, staged, nmaps)
        with torch.cuda.device(self.dev):
            if device_batch is None:
                self.desc.copy_(slot.desc, non_blocking=True)
                self.frames[:nbytes].copy_(slot.frames[:nbytes], non_blocking=True)
                if nmaps:
                    gf, gm = slot.gt(self)
                    self.gt_flow[:nmaps].copy_(gf[:nmaps], non_blocking=True)
                    self.gt_mask[:nmaps].copy_(gm[:nmaps], non_blocking=True)
            return self._replay(slot, [(i, h, w) for i, (h, w) in enumerate(shapes)], nmaps, want, files)

    def _num_pictures(self, nmaps):
        """How many of the pictures a replay draws: the last two exist only with ground truth (pair mode) or with both
        directions (sequence mode)."""
        if self.sequence:
            return len(VISUAL_IMAGES) if self.seq_bidir else len(FlowVisual._fields)
        return len(VISUAL_IMAGES) if nmaps else len(FlowVisual._fields)

    def _copy_back(self, slot, want, nmaps):
        """Queue the copies of the outputs named in `want` into the slot's pinned buffers.  The scores come back whenever ground
        truth was staged, the occlusion counts only when it had two maps."""
        special = {'sums': nmaps > 0, 'counts': nmaps > 0, 'occ_counts': 'occ_counts' in want and nmaps == 2}
        nv = self._num_pictures(nmaps)
        for name, attr, *_ in output_buffers(self.B, self.Hmax, self.Wmax, self.track_cap, self.interpolate, True, held_out=True,
                                                 stabilise=True, denoise=True):
            if special.get(name, name in want):
                dst, src = getattr(slot, name), getattr(self, attr)
                if name == 'vis':
                    dst, src = dst[:nv], src[:nv]
                dst.copy_(src, non_blocking=True)

    def _replay(self, slot, rows, nmaps, want, files):
        """What every replay ends with, once its inputs are staged and their copies queued: run, queue the copies back, the files'
        scanlines (_filter), and record the slot's event behind the last of them.  rows: [(slot row i, h, w), ...] of the
        replay's pairs — with nmaps, slot.pending, all the caller of a finished replay needs to know about it.  files: None, or
        (a function (rows, nmaps) -> _filter's entries, deflate) — the scanlines of those files come back in slot.scan."""
        self._run()
        self._copy_back(slot, want, nmaps)
        if files is not None:
            self._filter(slot, files[0](rows, nmaps), files[1])
        slot.event = torch.cuda.Event()
        slot.event.record(torch.cuda.current_stream(self.dev))
        slot.pending = (rows, nmaps)
        return slot

    @staticmethod
    def _one_ahead(submitted):
        """Yields (slot, rows, nmaps) of every replay of `submitted` (an iterator that submits a replay per step and yields its
        slot), in order and finished; replay k + 1 is staged and queued before replay k is handed to the caller, so host
        packing overlaps the device."""
        def finished(slot):
            slot.wait()
            return (slot,) + slot.pending
        prev = None
        for slot in submitted:
            if prev is not None:
                yield finished(prev)
            prev = slot
        if prev is not None:
            yield finished(prev)

    def _pipeline(self, batches, staged=None, nmaps_of=lambda b: 0, want=('flow',), files=None):
        """_one_ahead over batches of host examples."""
        return self._one_ahead(self._submit(k, exs, staged, nmaps_of(exs), want, files=files) for k, exs in enumerate(batches))

    # ------------------------------------------------------------------------------------------ public API
    def _mode(self, what, sequence, bidirectional=False, visual=False, track=False, interpolate=False, ground_truth=False,
              held_out=False, stabilise=False, denoise=False):
        """The guard of public method `what`: RuntimeError unless this is a pair (sequence False) or a sequence estimator, and
        one built with both directions / with pictures where the method needs them; the message names the constructor flags."""
        if not sequence:
            if self.sequence:
                raise RuntimeError("%s: a sequence estimator takes the frames of a clip (push, estimate_sequence, "
                                   "export_sequence); build a pair estimator without sequence=True" % what)
            if bidirectional and not self.bidirectional:
                raise RuntimeError("%s: a one-direction estimator; build it with FlowEstimator(..., bidirectional=True)" % what)
            if visual and not self.visual:
                raise RuntimeError("%s: an estimator without pictures; build it with FlowEstimator(..., visual=True)" % what)
            return
        if bidirectional and not self.seq_bidir:
            raise RuntimeError("%s: %s; build it with FlowEstimator(..., sequence='bidirectional')"
                               % (what, "a one-direction sequence estimator" if self.sequence else "a pair estimator"))
        if not self.sequence:
            raise RuntimeError("%s: a pair estimator; build it with FlowEstimator(..., sequence=True)" % what)
        if visual and not self.visual:
            raise RuntimeError("%s: a sequence estimator without pictures; build it with %s" % (what, self._visual_spelling()))
        if track and not self.track:
            raise RuntimeError("%s: a sequence estimator without tracks; build it with FlowEstimator(..., sequence=%r, track=True) "
                               "(or track=S, a grid stride, or track=anchors, an int array [N][2] of (x, y))"
                               % (what, 'bidirectional' if self.seq_bidir else True))
        if interpolate and not self.interpolate:
            raise RuntimeError("%s: a sequence estimator without in-between frames; build it with FlowEstimator(..., sequence=%r, "
                               "interpolate=n), n in 1..7" % (what, 'bidirectional' if self.seq_bidir else True))
        if ground_truth and not self.ground_truth:
            raise RuntimeError("%s: a sequence estimator without ground truth; build it with FlowEstimator(..., sequence=%r, "
                               "ground_truth=True)" % (what, 'bidirectional' if self.seq_bidir else True))
        if held_out and not self.held_out:
            raise RuntimeError("%s: a sequence estimator without held-out frames; build it with FlowEstimator(..., sequence=%r, "
                               "interpolate=n, held_out=True)" % (what, 'bidirectional' if self.seq_bidir else True))
        if stabilise and not self.stabilise:
            raise RuntimeError("%s: a sequence estimator without camera motion; build it with FlowEstimator(..., sequence=%r, "
                               "stabilise=True) (or stabilise=dict(tol=2, iters=3, follow=0))"
                               % (what, 'bidirectional' if self.seq_bidir else True))
        if denoise and not self.denoise:
            raise RuntimeError("%s: a sequence estimator without denoising; build it with FlowEstimator(..., "
                               "sequence='bidirectional', denoise=True) (or denoise=dict(tol='auto', depth=8))" % what)

    def _visual_spelling(self):
        """How to build this sequence estimator with pictures, for the messages that ask for it."""
        return "FlowEstimator(..., sequence=%r, visual='sequence')" % ('bidirectional' if self.seq_bidir else True)

    @staticmethod
    def _flows_of(slot, rows):
        """The rows of a finished replay as [h, w, 2] float32 flows (copies: the slot's buffers are overwritten two replays on)."""
        return [slot.flow.numpy()[i, :h, :w].copy() for i, h, w in rows]

    @staticmethod
    def _bidirectional_of(slot, rows):
        """The rows of a finished bidirectional replay as BidirectionalFlow tuples."""
        fl, fb, oc = slot.flow.numpy(), slot.flow_bw.numpy(), slot.occ.numpy()
        return [BidirectionalFlow(fl[i, :h, :w].copy(), fb[i, :h, :w].copy(), oc[0, i, :h, :w].astype(bool),
                                  oc[1, i, :h, :w].astype(bool)) for i, h, w in rows]

    @staticmethod
    def _visual_of(slot, rows, kind=FlowVisual):
        """The rows of a finished visual replay as tuples of pictures: FlowVisual, or SequenceVisual with both directions."""
        v = slot.vis.numpy()
        return [kind(*(v[k, i, :h, :w].copy() for k in range(len(kind._fields)))) for i, h, w in rows]

    @staticmethod
    def _pairs(frames1, frames2, what):
        if len(frames1) != len(frames2):
            raise ValueError("%s: %d first frames, %d second frames" % (what, len(frames1), len(frames2)))
        exs = []
        for a, b in zip(frames1, frames2):
            a = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
            b = np.asarray(b.cpu().numpy() if isinstance(b, torch.Tensor) else b)
            if a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("%s: a pair must be two [h, w, 3] frames of one size, got %s and %s" % (what, a.shape, b.shape))
            if a.dtype != np.uint8:
                a, b = a.astype(np.float32, copy=False), b.astype(np.float32, copy=False)
            exs.append((a, b, a.shape[:2]))
        return exs

    def estimate(self, frames1, frames2):
        """Flow of every pair (frames1[i] -> frames2[i]): frames [h_i, w_i, 3] uint8 or float32 in [0, 255], any size up to
        max_frame (both frames of a pair the same size).  Returns a list of [h_i, w_i, 2] float32 arrays."""
        self._mode('estimate', sequence=False)
        exs = self._pairs(frames1, frames2, 'estimate')
        out = []
        for slot, rows, _ in self._pipeline(chunks(exs, self.B)):
            out += self._flows_of(slot, rows)
        return out

    def estimate_bidirectional(self, frames1, frames2):
        """estimate's pairs in both directions: one BidirectionalFlow(flow_fw, flow_bw, occ_fw, occ_bw) per pair — the flows
        [h_i, w_i, 2] float32 (flow_fw = estimate's flow), the masks [h_i, w_i] bool: losses.occlusion(flow_fw, flow_bw)."""
        self._mode('estimate_bidirectional', sequence=False, bidirectional=True)
        exs = self._pairs(frames1, frames2, 'estimate_bidirectional')
        out = []
        for slot, rows, _ in self._pipeline(chunks(exs, self.B), want=('flow', 'flow_bw', 'occ')):
            out += self._bidirectional_of(slot, rows)
        return out

    def visualize(self, frames1, frames2):
        """estimate's pairs as pictures: one FlowVisual(overlay, warp_error, flow) per pair, uint8 [h_i, w_i, 3] — the slots of
        eval_gui.py:199-204 (:160-165): (0.5 im1 + 0.5 im2) / 255 and |im1 - image_warp(im2, flow)| / 255 on the frames as the
        reference shows them (resized to the network's size and back), and flow_to_color(flow) with max_flow per pair; bytes
        rounded to nearest."""
        self._mode('visualize', sequence=False, visual=True)
        exs = self._pairs(frames1, frames2, 'visualize')
        out = []
        for slot, rows, _ in self._pipeline(chunks(exs, self.B), want=('vis',)):
            out += self._visual_of(slot, rows)
        return out

    def pictures(self, batch_iter, num=None, scanlines=False, deflate='host'):
        """The pictures of what KITTIInput.input_{train,test}_{2012,2015}() yields, one dict per example in iteration order:
        VISUAL_IMAGES' names -> uint8 [h, w, 3]; 'error' and 'gt' only when the input carries ground truth (two maps:
        flow_error_image(flow, flow_occ, mask_occ, mask_noc) and flow_to_color(flow_occ, mask_occ); one map: mask_noc = ones).
        scanlines: every dict also has 'scanlines': image name -> (h, w, depth, colour type, bytes), the picture's finished PNG
        scanlines from the device encode path (unflow_png_filter), what png_device.DeviceFileWriter.submit takes.
        deflate='device' (with scanlines): the bytes are the scanlines' finished zlib stream instead (unflow_deflate), and
        'scanlines_kind' is 'png_z', the kind to submit them as ('png' otherwise)."""
        from .png_device import check_deflate_mode
        self._mode('pictures', sequence=False)
        on_device = check_deflate_mode(deflate)
        if on_device and not scanlines:
            raise ValueError("pictures: deflate='device' codes the scanlines; it needs scanlines=True")
        self._mode('pictures', sequence=False, visual=True)
        B, files = self.B, None
        if scanlines:         # per example its pictures by index, the order of the dict below: not the order of export's files
            def entries(rows, nmaps):
                return [('vis', k * B + i, h, w) for i, h, w in rows for k in range(self._num_pictures(nmaps))]
            files = (entries, on_device)
        for slot, rows, nmaps in self._staged_input(batch_iter, num, ('vis',), lambda exs: (len(exs[0]) - 3) // 2, files):
            v = slot.vis.numpy()
            spans = iter(slot.spans or ())
            for i, h, w in rows:
                ex = {name: v[k, i, :h, :w].copy() for k, name in enumerate(VISUAL_IMAGES[:self._num_pictures(nmaps)])}
                if scanlines:
                    sc, buf = {}, slot.scan.numpy()
                    for name in ex:
                        off, nb, _, _, depth, ctype = next(spans)
                        sc[name] = (h, w, depth, ctype, buf[off:off + nb].tobytes())
                    ex['scanlines'] = sc
                    ex['scanlines_kind'] = slot.scan_kind
                yield ex

    def evaluate(self, batch_iter, num=None):
        """Scores on what KITTIInput.input_train_{2012,2015}() yields — (im1, im2, input_shape, flow_occ, mask_occ, flow_noc,
        mask_noc) — or the 2-map form (im1, im2, input_shape, flow_gt, mask), any batch size.  The frames are the
        KITTIInput layout (cropped / padded to its dims, normalize=False); the flow is scored at each frame's own size
        against the ground truth cropped back the same way (Trainer.eval's chain).  Returns the per-example averages of
        AEE/<map> and outliers/<map> (%) — map = occluded, non-occluded (or all) — num_examples and per_example (rows in
        `names` order).  num: at most that many examples.
        A bidirectional estimator on two-map input adds occlusion_scores' occ/precision, occ/recall and occ/F1 (%, pooled
        over all examples) and occ_counts (per example [tp, fp, fn])."""
        self._mode('evaluate', sequence=False)
        names, rows, occ_rows = None, [], []
        want = ('occ_counts',) if self.bidirectional else ()
        for slot, pairs, nmaps in self._staged_input(batch_iter, num, want, lambda exs: (len(exs[0]) - 3) // 2):
            if nmaps == 0:
                raise ValueError("evaluate: the batches carry no ground truth (a test split); use export()")
            if names is None:
                names = [n for m in MAP_NAMES[nmaps] for n in ('AEE/' + m, 'outliers/' + m)]
            sums, counts = slot.sums.numpy(), slot.counts.numpy()
            for i, _, _ in pairs:
                row = []
                for m in range(nmaps):
                    err, msk = float(sums[i, m, 0]), float(sums[i, m, 1])
                    row += [err / msk, 100.0 * float(counts[i, m]) / msk]
                rows.append(row)
            if self.bidirectional and nmaps == 2:
                occ_rows += [[int(v) for v in slot.occ_counts.numpy()[i]] for i, _, _ in pairs]
        if not rows:
            raise ValueError("evaluate: the input yielded no examples")
        avg = np.mean(np.asarray(rows, dtype=np.float64), axis=0)
        out = {k: float(v) for k, v in zip(names, avg)}
        out.update(num_examples=len(rows), per_example=rows, names=names)
        if occ_rows and len(occ_rows) == len(rows):
            out.update(occlusion_scores(occ_rows))
            out['occ_counts'] = occ_rows
        return out

    def _staged_examples(self, it):
        """Examples of the KITTIInput layout (all cropped / padded to one size): that size is remembered for the origins of the
        descriptor table."""
        for ex in it:
            dims = np.asarray(ex[0]).shape[:2]
            if self._dims is None:
                self._dims = dims
            elif tuple(dims) != tuple(self._dims):
                raise ValueError("evaluate / export: the input's frames changed size (%s, then %s)" % (self._dims, dims))
            yield ex

    def _pipeline_staged(self, it, want, nmaps_of, files=None):
        """_pipeline over examples of the KITTIInput layout."""
        self._dims = None
        gen = self._staged_examples(it)
        first = next(gen, None)
        if first is None:
            return
        batches = chunks(itertools.chain([first], gen), self.B)
        yield from self._pipeline(batches, staged=tuple(self._dims), nmaps_of=nmaps_of, want=want, files=files)

    def _on_device(self, batch):
        t = batch[0]
        return isinstance(t, torch.Tensor) and t.is_cuda and \
            t.device == torch.device('cuda', torch.cuda.current_device() if self.dev.index is None else self.dev.index)

    def _pipeline_device(self, batches, num, want, nmaps_of, files=None):
        """_one_ahead over batches of device tensors (DeviceEvalBatches): each is consumed as it comes, never re-chunked —
        its tensors are valid only until the iterator's next next(), and batch k is staged (copies enqueued on the current
        stream) before batch k + 1 is asked for."""
        def replays():
            self._dims = None
            done = 0
            for k, batch in enumerate(batches):
                if len(batch) not in (3, 5, 7):
                    raise ValueError("a batch is (im1, im2, input_shape) + 0, 1 or 2 (flow, mask) pairs; got %d arrays" % len(batch))
                n = int(batch[0].shape[0])
                if n > self.B:
                    raise ValueError("a device batch of %d examples for an estimator of batch %d: device batches are consumed "
                                     "whole (build the input with batch_size <= %d)" % (n, self.B, self.B))
                if num is not None:
                    n = min(n, int(num) - done)
                    if n <= 0:
                        return
                dims = tuple(int(v) for v in batch[0].shape[1:3])
                if self._dims is None:
                    self._dims = dims
                elif dims != tuple(self._dims):
                    raise ValueError("evaluate / export: the input's frames changed size (%s, then %s)" % (self._dims, dims))
                done += n
                yield self._submit(k, None, dims, nmaps_of([batch]), want, device_batch=(batch, n), files=files)
        return self._one_ahead(replays())

    def _staged_input(self, batch_iter, num, want, nmaps_of, files=None):
        """The batches of evaluate / export / pictures: host arrays go example by example through _pipeline_staged; batches of
        tensors on this estimator's device through _pipeline_device."""
        batch_iter = iter(batch_iter)
        first = next(batch_iter, None)
        if first is None:
            return
        batches = itertools.chain([first], batch_iter)
        if self._on_device(first):
            yield from self._pipeline_device(batches, num, want, nmaps_of, files)
            return
        it = example_stream(batches)
        if num is not None:
            it = (ex for i, ex in zip(range(int(num)), it))
        yield from self._pipeline_staged(it, want, nmaps_of, files)

    def export(self, batch_iter, out_dir, fmt='png', num=None, backward=False, occlusion=False, visual=False, workers=0,
               level=6, deflate='host'):
        """The benchmark files of eval_gui.py --output_benchmark (:247-263): for the k-th example in iteration order,
        out_dir/%06d_10.png (KITTI 16-bit RGB, --output_png) or out_dir/%06d_10.flo.  Input: what
        KITTIInput.input_{train,test}_{2012,2015}() yields.  Returns the written paths (per example: _10, _01, _10_occ, then
        the pictures).
        backward: also the backward flow, %06d_01.png / .flo (the file eval_gui.py --output_backward means); occlusion: the
        forward occlusion mask, %06d_10_occ.png (8-bit grey, 255 = occluded).  Both need a bidirectional estimator.
        visual (an estimator built with visual=True): after those, the 8-bit pictures of eval_gui.py --output_visual:
        %06d_img.png (overlay), %06d_flow.png (flow colours), %06d_diff.png (brightness error) and, when the input carries
        ground truth (two maps or one), %06d_err.png (the KITTI error image) and %06d_gt.png (the ground truth's colours).
        eval_gui.py:248-254 writes the brightness error into _flow.png and the flow colours into _err.png and never writes the
        error image; the names' evident meaning is followed here.
        workers = 0 (the default): the host writers of core/input.py, one file after another on this thread (filter 0 on every
        row).  workers >= 1: the device encode path — unflow_png_filter chooses and applies a filter per row right
        behind each replay, the scanlines come back instead of the raw outputs, and a pool of `workers` threads
        (png_device.DeviceFileWriter) deflates at `level` and writes; .flo files go through the same pool.  The same paths in
        the same order, files that decode to the same pixels (.flo: the same bytes), all written when the call returns.
        deflate='device' (needs workers >= 1): the scanlines are deflated on the device as well (unflow_deflate,
        right behind the filter launch, outside the captured graph), only the zlib streams come back and the pool's threads form
        the chunk CRCs and write; `level` does not apply.  .flo files are not compressed and go the same way as before."""
        from .png_device import check_deflate_mode
        self._mode('export', sequence=False)
        on_device = check_deflate_mode(deflate, workers)
        if fmt not in ('png', 'flo'):
            raise ValueError("export: fmt must be 'png' or 'flo'")
        if (backward or occlusion) and not self.bidirectional:
            raise ValueError("export: backward / occlusion files need FlowEstimator(..., bidirectional=True)")
        if visual and not self.visual:
            raise ValueError("export: the pictures need FlowEstimator(..., visual=True)")
        # the ground truth is staged only for the pictures that show it
        nmaps_of = (lambda exs: (len(exs[0]) - 3) // 2) if visual else (lambda exs: 0)

        def plan(n, nmaps):
            return pair_files(n, fmt, backward, occlusion, visual_files(n, nmaps > 0) if visual else ())       # _img .. _gt
        return self._write_files(lambda want, files: self._staged_input(batch_iter, num, want, nmaps_of, files), plan, out_dir,
                                 workers, level, on_device)

    def _write_files(self, replays, plan, out_dir, workers, level, deflate):
        """The files of export / export_sequence, pair after pair.  plan: (pair number n, nmaps) -> pair_files' list for that
        pair; replays: (want, files) -> the finished replays (_one_ahead's) of a pass submitted with those two.  Returns the paths
        in the order written.
        workers = 0: the outputs the plan names come back raw and the host writers of core/input.py write them on this thread.
        workers >= 1: the plan's PNGs are the entries of each replay's unflow_png_filter launch (filter_entries: the same list,
        so slot.spans is in file order), only their scanlines (deflate: zlib streams) and the .flo flows come back, and a
        png_device.DeviceFileWriter pool finishes and writes them; every file is written when this returns."""
        from .input import write_flo, write_kitti_flow_png, write_png_gray8, write_png_rgb8
        from .png_device import DeviceFileWriter, flo_file_bytes
        os.makedirs(out_dir, exist_ok=True)
        want = tuple(src[1] for _, src in plan(0, 0) if not workers or src[0] in ('flo', 'track'))
        want += ('track_alive',) if 'track_disp' in want else ()
        files = (lambda rows, nmaps: filter_entries(plan(0, nmaps), rows, self.B), deflate) if workers else None
        pool = DeviceFileWriter(workers, level) if workers else None
        paths, n = [], 0
        with contextlib.nullcontext() if pool is None else pool:
            for slot, rows, nmaps in replays(want, files):
                spans = iter(slot.spans or ())
                for i, h, w in rows:
                    for name, (kind, attr, *k) in plan(n, nmaps):
                        path = os.path.join(out_dir, name)
                        if kind == 'track':
                            grid = self._track_flo(slot, i, h, w)
                            if pool is not None:
                                pool.submit(path, 'flo', flo_file_bytes(grid))
                            else:
                                write_flo(path, grid)
                        elif pool is not None and kind == 'png':
                            off, nb, _, _, depth, ctype = next(spans)
                            pool.submit(path, slot.scan_kind, (h, w, depth, ctype, slot.scan.numpy()[off:off + nb].tobytes()))
                        elif pool is not None:
                            pool.submit(path, 'flo', flo_file_bytes(getattr(slot, attr).numpy()[i, :h, :w]))
                        elif kind == 'flo':
                            write_flo(path, getattr(slot, attr).numpy()[i, :h, :w])
                        elif attr == 'occ':
                            write_png_gray8(path, slot.occ.numpy()[0, i, :h, :w] * np.uint8(255))
                        elif attr == 'vis':
                            write_png_rgb8(path, slot.vis.numpy()[k[0], i, :h, :w])
                        elif attr == 'mid':
                            write_png_rgb8(path, slot.mid.numpy()[k[0], i, :h, :w])
                        elif attr == 'stab':
                            write_png_rgb8(path, slot.stab.numpy()[i, :h, :w])
                        elif attr == 'stab_resid':
                            write_png_gray8(path, slot.stab_resid.numpy()[i, :h, :w])
                        elif attr == 'den':
                            write_png_rgb8(path, slot.den.numpy()[i, :h, :w])
                        else:
                            write_kitti_flow_png(path, getattr(slot, attr).numpy()[i, :h, :w].view(np.uint16))
                        paths.append(path)
                    n += 1
        return paths

    # ------------------------------------------------------------------------------------------ sequence mode
    def reset(self):
        """Start a new clip: the next push has no previous frame (nothing is carried across reset)."""
        self._mode('reset', sequence=True)
        self._carry, self._clip = 0, None
        self._max_flow = _UNSET
        self._clip_nmaps = 0

    def _clip_max_flow(self, max_flow, what):
        """The max_flow of the clip's flow colours: taken from the call that starts the clip (None: a maximum per pair); a later
        call may repeat it or leave it out."""
        if max_flow is not None:
            max_flow = float(max_flow)
            if not self.visual:
                raise RuntimeError("%s: max_flow scales the flow colours; build the estimator with %s"
                                   % (what, self._visual_spelling()))
        if self._max_flow is _UNSET:
            self._max_flow = max_flow
        elif max_flow is not None and max_flow != self._max_flow:
            raise ValueError("%s: max_flow belongs to the clip (%s since its first frames, now %s); reset() starts a new clip"
                             % (what, self._max_flow, max_flow))
        return self._max_flow

    def _clip_frames(self, frames, what):
        out = []
        for a in frames:
            if isinstance(a, torch.Tensor) and self._on_device((a,)):      # stays on the device: staged with a device copy
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError("%s: a frame is [h, w, 3], got %s" % (what, tuple(a.shape)))
                if a.dtype != torch.uint8:
                    a = a.float()
                u8 = a.dtype == torch.uint8
            else:
                a = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError("%s: a frame is [h, w, 3], got %s" % (what, a.shape))
                if a.dtype != np.uint8:
                    a = a.astype(np.float32, copy=False)
                u8 = a.dtype == np.uint8
            clip = (int(a.shape[0]), int(a.shape[1]), bool(u8))
            if clip[0] > self.Hmax or clip[1] > self.Wmax:
                raise ValueError("%s: a %dx%d frame exceeds max_frame %dx%d" % (what, clip[0], clip[1], self.Hmax, self.Wmax))
            if self._clip is None:
                self._clip = clip
            elif clip != self._clip:
                raise ValueError("%s: the frames of a clip have one size and type (%s, then %s); reset() starts a new clip"
                                 % (what, self._clip, clip))
            out.append(a)
        return out

    def _clip_gts(self, gts, n_frames, what):
        """The ground truth of a scored push, checked before anything is staged: gts[i] belongs to the pair that ends at the
        i-th new frame — None for a clip's first frame only, else (flow, mask) or (flow_occ, mask_occ, flow_noc, mask_noc), one
        map count per clip.  Returns [None | [(flow [h, w, 2], mask [h, w]), ...]] with host arrays as float32 numpy, tensors on
        this device left where they are."""
        gts = list(gts)
        if len(gts) != n_frames:
            raise ValueError("%s: %d frames, %d ground truths (one per frame; None for a clip's first frame)"
                             % (what, n_frames, len(gts)))
        h, w, _ = self._clip
        out = []
        for i, g in enumerate(gts):
            first = self._carry == 0 and i == 0
            if g is None:
                if not first:
                    raise ValueError("%s: frame %d has no ground truth; only a clip's first frame ends no pair" % (what, i))
                out.append(None)
                continue
            if len(g) not in (2, 4):
                raise ValueError("%s: the ground truth of frame %d is (flow, mask) or (flow_occ, mask_occ, flow_noc, mask_noc), "
                                 "got %d arrays" % (what, i, len(g)))
            if first:                             # the pair that would end here does not exist: nothing to score
                out.append(None)
                continue
            nmaps = len(g) // 2
            if self._clip_nmaps == 0:
                self._clip_nmaps = nmaps
            elif nmaps != self._clip_nmaps:
                raise ValueError("%s: the ground truth of frame %d has %d map(s), the clip's has %d; reset() starts a new clip"
                                 % (what, i, nmaps, self._clip_nmaps))
            maps = []
            for m in range(nmaps):
                f, msk = g[2 * m], g[2 * m + 1]
                if not (isinstance(f, torch.Tensor) and self._on_device((f,))):
                    f = np.asarray(f.cpu().numpy() if isinstance(f, torch.Tensor) else f, dtype=np.float32)
                if not (isinstance(msk, torch.Tensor) and self._on_device((msk,))):
                    msk = np.asarray(msk.cpu().numpy() if isinstance(msk, torch.Tensor) else msk, dtype=np.float32)
                if tuple(f.shape) != (h, w, 2) or tuple(msk.shape) not in ((h, w), (h, w, 1)):
                    raise ValueError("%s: the ground truth of frame %d is a [%d, %d, 2] flow and a [%d, %d] mask, got %s and %s"
                                     % (what, i, h, w, h, w, tuple(f.shape), tuple(msk.shape)))
                maps.append((f, msk.reshape(h, w)))
            out.append(maps)
        return out

    def _stage_gts(self, slot, gts, h, w):
        """Ground truth of pair slot i = gts[i], at the origin of its row, zero outside (h, w): host arrays through the slot's
        pinned buffers and one upload, tensors of this device by device copies behind it (as _submit_sequence's frames)."""
        nmaps = self._clip_nmaps
        gf, gm = slot.gt(self)
        host = False
        for i, maps in enumerate(gts):
            for m, (f, msk) in enumerate(maps or ()):
                if isinstance(f, torch.Tensor) and isinstance(msk, torch.Tensor):
                    continue
                host = True
                for dst, src in ((gf[m, i].numpy(), f), (gm[m, i].numpy(), msk)):
                    if not isinstance(src, torch.Tensor):
                        dst[:h, :w] = src
                        dst[h:] = 0
                        dst[:h, w:] = 0
        with torch.cuda.device(self.dev):
            if host:
                self.gt_flow[:nmaps].copy_(gf[:nmaps], non_blocking=True)
                self.gt_mask[:nmaps].copy_(gm[:nmaps], non_blocking=True)
            for i, maps in enumerate(gts):
                for m, (f, msk) in enumerate(maps or ()):
                    for dst, src in ((self.gt_flow[m, i], f), (self.gt_mask[m, i], msk)):
                        if isinstance(src, torch.Tensor):
                            dst[:h, :w].copy_(src.float(), non_blocking=True)
                            dst[h:].zero_()
                            dst[:h, w:].zero_()

    def _clip_truths(self, truths, n_frames, what):
        """The held-out frames of a push, checked before anything is staged: truths[i] holds the n frames between the frame before
        the i-th new frame and it — n [h, w, 3] arrays or one [n, h, w, 3], of the clip's size and dtype; None for a clip's first
        frame only.  Returns [None | [n frames]], host arrays as numpy, tensors of this device left where they are."""
        truths = list(truths)
        if len(truths) != n_frames:
            raise ValueError("%s: %d frames, %d sets of held-out frames (one per frame; None for a clip's first frame)"
                             % (what, n_frames, len(truths)))
        h, w, u8 = self._clip
        n, out = self.interpolate, []
        for i, t in enumerate(truths):
            first = self._carry == 0 and i == 0
            if t is None:
                if not first:
                    raise ValueError("%s: frame %d has no held-out frames; only a clip's first frame ends no pair" % (what, i))
                out.append(None)
                continue
            if len(t) != n:
                raise ValueError("%s: frame %d comes with %d held-out frames, the estimator interpolates %d per pair"
                                 % (what, i, len(t), n))
            got = []
            for a in t:
                if not (isinstance(a, torch.Tensor) and self._on_device((a,))):
                    a = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
                a_u8 = a.dtype == (torch.uint8 if isinstance(a, torch.Tensor) else np.uint8)
                if tuple(a.shape) != (h, w, 3) or a_u8 != u8:
                    raise ValueError("%s: the held-out frames of frame %d have the clip's size and type ([%d, %d, 3] %s), got %s %s"
                                     % (what, i, h, w, 'uint8' if u8 else 'float32', tuple(a.shape), a.dtype))
                if not u8:
                    a = a.float() if isinstance(a, torch.Tensor) else a.astype(np.float32, copy=False)
                got.append(a)
            out.append(None if first else got)       # the pair that would end at a clip's first frame does not exist
        return out

    def _stage_truths(self, slot, truths, h, w, u8):
        """Truth frame j of pair slot i = truths[i][j - 1] at [j - 1][i], at the origin: host arrays through the slot's pinned buffer
        and one upload, tensors of this device by device copies behind it (as the frames)."""
        n, B, Hm, Wm = self.interpolate, self.B, self.Hmax, self.Wmax
        nbytes = n * B * Hm * Wm * 3 * (1 if u8 else 4)
        pinned = slot.truth[:nbytes].numpy().view(np.uint8 if u8 else np.float32).reshape(n, B, Hm, Wm, 3)
        on_dev, host = [], False
        for i, t in enumerate(truths):
            for j, a in enumerate(t or ()):
                if isinstance(a, torch.Tensor):
                    on_dev.append((j, i, a))
                else:
                    pinned[j, i, :h, :w] = a
                    host = True
        with torch.cuda.device(self.dev):
            if host:
                self.mid_truth[:nbytes].copy_(slot.truth[:nbytes], non_blocking=True)
            dv = self.mid_truth[:nbytes].view(torch.uint8 if u8 else torch.float32).view(n, B, Hm, Wm, 3)
            for j, i, a in on_dev:
                dv[j, i, :h, :w].copy_(a, non_blocking=True)

    def _submit_sequence(self, frames, want=('flow',), files=None, max_flow=None, gts=None, truths=None):
        """Stage 1..B new frames of the clip, copy them and the tables in, run, queue the copies back; returns the slot, its
        rows the valid pair slots.  want: the outputs to copy back ('flow', 'u16'; bidirectional: 'flow_bw', 'u16_bw', 'occ';
        visual: 'vis'); files: _replay's.  max_flow: the clip's (_clip_max_flow).  gts (an estimator with ground_truth): the
        ground truth per new frame (_clip_gts); the pairs are then scored and slot.pending carries their map count.  truths (an
        estimator with held_out): the held-out frames per new frame (_clip_truths); the tables then say held and the in-between
        frames are scored."""
        B, Hm, Wm = self.B, self.Hmax, self.Wmax
        if not 1 <= len(frames) <= B:
            raise ValueError("push: 1 to %d new frames per replay, got %d" % (B, len(frames)))
        max_flow = self._clip_max_flow(max_flow, 'push')
        frames = self._clip_frames(frames, 'push')
        h, w, u8 = self._clip
        if gts is not None:
            gts = self._clip_gts(gts, len(frames), 'push_scored')
        nmaps = self._clip_nmaps if gts is not None else 0
        if truths is not None:
            truths = self._clip_truths(truths, len(frames), 'push_held_out')
        slot = self._slot(self._seq_k)
        self._seq_k += 1
        slot.wait()
        nbytes = B * Hm * Wm * 3 * (1 if u8 else 4)
        fr = slot.frames[:nbytes].numpy().view(np.uint8 if u8 else np.float32).reshape(B, Hm, Wm, 3)
        on_dev = [(i, a) for i, a in enumerate(frames) if isinstance(a, torch.Tensor)]
        for i, a in enumerate(frames):
            if not isinstance(a, torch.Tensor):
                fr[i, :h, :w] = a
        starts = self._carry == 0                 # the clip's first replay
        tab, valid, self._carry = sequence_tables((h, w), len(frames), B, self._carry, u8, max_flow, self._track_words(h, w),
                                                  nmaps=nmaps, held=int(truths is not None))
        slot.tab.numpy()[:] = tab
        if nmaps:
            self._stage_gts(slot, gts, h, w)
        if truths is not None:
            self._stage_truths(slot, truths, h, w, u8)
        with torch.cuda.device(self.dev):
            self.tab.copy_(slot.tab, non_blocking=True)
            if len(on_dev) < len(frames):
                self.frames[:nbytes].copy_(slot.frames[:nbytes], non_blocking=True)
            if on_dev:                            # frames already on this device: device copies behind the upload, no host trip
                dv = self.frames[:nbytes].view(torch.uint8 if u8 else torch.float32).view(B, Hm, Wm, 3)
                for i, a in on_dev:
                    dv[i, :h, :w].copy_(a, non_blocking=True)
            if self.stabilise and starts and not valid:
                # a clip that starts with one frame: its replay has no pair and unflow_sequence_stabilise leaves the path alone,
                # the next one carries and continues from it — from the identity, not from the last clip's path (a device copy
                # in front of the replay, outside the graph)
                self.stab_path.copy_(self.stab_identity, non_blocking=True)
            return self._replay(slot, [(i, h, w) for i in valid], nmaps, want, files)

    def _push(self, frames, want, max_flow=None):
        """One replay on its own: (slot, rows) once it has finished."""
        slot = self._submit_sequence(list(frames), want, max_flow=max_flow)
        slot.wait()
        return slot, slot.pending[0]

    def push(self, frames):
        """The next 1..B frames of the clip ([h, w, 3] uint8 or float32 in [0, 255], all of the clip's size).  Returns one
        [h, w, 2] float32 flow per new pair, in order: from the frame before each new frame to it — len(frames) flows, or
        len(frames) - 1 for the first push after reset() (its first frame has no predecessor)."""
        self._mode('push', sequence=True)
        return self._flows_of(*self._push(frames, ('flow',)))

    def push_bidirectional(self, frames):
        """push on a sequence='bidirectional' estimator, both directions: one BidirectionalFlow(flow_fw, flow_bw, occ_fw, occ_bw)
        per new pair (n, n + 1) — flow_fw from frame n to n + 1 (push's flow), flow_bw from frame n + 1 to n, the masks
        losses.occlusion of the two, as estimate_bidirectional returns them.  The count is push's."""
        self._mode('push_bidirectional', sequence=True, bidirectional=True)
        return self._bidirectional_of(*self._push(frames, ('flow', 'flow_bw', 'occ')))

    def estimate_sequence_bidirectional(self, frames):
        """estimate_sequence in both directions: T >= 2 frames -> T - 1 BidirectionalFlow tuples (push_bidirectional's)."""
        self._mode('estimate_sequence_bidirectional', sequence=True, bidirectional=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, ('flow', 'flow_bw', 'occ')):
            out += self._bidirectional_of(slot, rows)
        return out

    def push_visual(self, frames, max_flow=None):
        """push's frames as pictures: one tuple of uint8 [h, w, 3] images per new pair (the count is push's) — visualize's
        FlowVisual(overlay, warp_error, flow), every frame of the clip resampled once; on a sequence='bidirectional' estimator
        SequenceVisual(overlay, warp_error, flow, flow_bw, warp_error_noc): also flow_to_color of the backward flow (its own
        maximum) and the brightness error where the forward occlusion mask is 0, black where it is 1.
        max_flow: the scale of the flow colours (used as max(max_flow, 1)) for the whole clip, taken from the first push after
        reset(); None: every pair has its own maximum, as in pair mode.  Another value later in the clip: ValueError."""
        self._mode('push_visual', sequence=True, visual=True)
        return self._visual_of(*self._push(frames, ('vis',), max_flow), SequenceVisual if self.seq_bidir else FlowVisual)

    def visualize_sequence(self, frames, max_flow=None):
        """estimate_sequence's clip as pictures: T >= 2 frames -> T - 1 tuples (push_visual's), max_flow for the whole clip."""
        self._mode('visualize_sequence', sequence=True, visual=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, ('vis',), max_flow=max_flow):
            out += self._visual_of(slot, rows, SequenceVisual if self.seq_bidir else FlowVisual)
        return out

    # tracks
    def _track_shape(self, h, w):
        """The shape of one pair's tracks for a clip of (h, w) frames: the dense grid (gh, gw), or (N,) with sparse anchors."""
        kind, arg = self.track_spec
        return track_grid((h, w), arg) if kind == 'dense' else (int(arg.shape[0]),)

    def _track_words(self, h, w):
        """(S, N) for sequence_tables: the grid stride (0: sparse anchors) and the number of tracks of a clip of (h, w) frames;
        None without tracks.  More tracks than the buffers hold: ValueError before the replay (the kernel would clamp)."""
        if not self.track:
            return None
        n = int(np.prod(self._track_shape(h, w)))
        if n > self.track_cap:
            raise ValueError("push: %d tracks on a %dx%d frame exceed the estimator's capacity of %d" % (n, h, w, self.track_cap))
        return (self.track_spec[1] if self.track_spec[0] == 'dense' else 0, n)

    def _tracks_of(self, slot, rows):
        """The rows of a finished tracking replay as Track tuples (copies)."""
        d, a = slot.track_disp.numpy(), slot.track_alive.numpy()
        out = []
        for i, h, w in rows:
            shape = self._track_shape(h, w)
            n = int(np.prod(shape))
            out.append(Track(d[i, :n].reshape(shape + (2,)).copy(), a[i, :n].reshape(shape).astype(bool)))
        return out

    def _track_flo(self, slot, i, h, w):
        """Row i of a finished tracking replay as the [gh, gw, 2] float32 array of %06d_track.flo: the displacement from the
        clip's first frame, (TRACK_DEAD, TRACK_DEAD) where the track is dead."""
        t, = self._tracks_of(slot, [(i, h, w)])
        return np.where(t.alive[..., None], t.disp, np.float32(TRACK_DEAD)).astype(np.float32)

    def push_tracks(self, frames):
        """push's frames on an estimator built with track: one Track(disp, alive) per new pair (the count is push's).  For the
        pair (n, n + 1), disp is where every anchor of the clip's first frame is in frame n + 1, as its displacement from the
        anchor — float32 [gh, gw, 2] on the dense grid (anchor (S gx, S gy) at [gy, gx]) or [N, 2] for sparse anchors — and alive
        bool [gh, gw] / [N]: still inside the frame and (sequence='bidirectional') never under a forward occlusion mask.  A dead
        track keeps the disp it had when it died."""
        self._mode('push_tracks', sequence=True, track=True)
        return self._tracks_of(*self._push(frames, ('track_disp', 'track_alive')))

    def track_sequence(self, frames):
        """Tracks along a clip: T >= 2 frames -> T - 1 Track tuples (push_tracks'), anchored in the first frame."""
        self._mode('track_sequence', sequence=True, track=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, ('track_disp', 'track_alive')):
            out += self._tracks_of(slot, rows)
        return out

    # in-between frames
    @staticmethod
    def _interpolated_of(slot, rows):
        """The rows of a finished interpolating replay as Interpolated tuples (copies)."""
        m, hl = slot.mid.numpy(), slot.mid_holes.numpy()
        return [Interpolated(m[:, i, :h, :w].copy(), hl[:, i].astype(np.int64)) for i, h, w in rows]

    def push_interpolated(self, frames):
        """push's frames on an estimator built with interpolate=n: one Interpolated(frames, holes) per new pair (the count is
        push's).  For the pair (k, k + 1), frames is uint8 [n, h, w, 3], in-between frame j = 1..n at time j / (n + 1) between the
        two staged frames — frame k's colours splatted along the forward flow and, on a sequence='bidirectional' estimator, frame
        k + 1's along the backward flow, occluded pixels unblended (unflow_sequence_interpolate) — and holes int [n], the pixels of
        each that no source reached and the temporal blend of the two frames fills.  Bit-reproducible from run to run."""
        self._mode('push_interpolated', sequence=True, interpolate=True)
        return self._interpolated_of(*self._push(frames, ('mid', 'mid_holes')))

    def interpolate_sequence(self, frames):
        """In-between frames along a clip: T >= 2 frames -> T - 1 Interpolated tuples (push_interpolated's)."""
        self._mode('interpolate_sequence', sequence=True, interpolate=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, ('mid', 'mid_holes')):
            out += self._interpolated_of(slot, rows)
        return out

    # camera motion
    STAB_WANT = ('stab', 'stab_resid', 'stab_motion', 'stab_path', 'stab_counts')

    @staticmethod
    def _stabilised_of(slot, rows):
        """The rows of a finished stabilising replay as Stabilised tuples (copies)."""
        s, r, m, p, c = (getattr(slot, name).numpy() for name in FlowEstimator.STAB_WANT)
        return [Stabilised(s[i, :h, :w].copy(), r[i, :h, :w].copy(), m[i].copy(), p[i].copy(), c[i].astype(np.int64))
                for i, h, w in rows]

    def push_stabilised(self, frames):
        """push's frames on an estimator built with stabilise: one Stabilised(frame, residual, motion, path, counts) per new pair
        (the count is push's).  For the pair (n, n + 1): motion, the robust affine fit to the forward flow (on a
        sequence='bidirectional' estimator the pixels under the forward occlusion mask are left out); residual, every pixel's
        distance from it in quarter pixels — the independently moving objects stand out; path, the camera path up to frame n + 1,
        the motions composed from the clip's first frame (with follow = s it drifts back to the identity by 2^-s per pair); frame,
        frame n + 1 resampled along that path — with follow = 0 in the first frame's coordinates — black where the path leaves
        the frame (counts[3] pixels).  Bit-reproducible from run to run.  reset() starts a new path."""
        self._mode('push_stabilised', sequence=True, stabilise=True)
        return self._stabilised_of(*self._push(frames, self.STAB_WANT))

    def stabilise_sequence(self, frames):
        """Camera motion along a clip: T >= 2 frames -> T - 1 Stabilised tuples (push_stabilised's)."""
        self._mode('stabilise_sequence', sequence=True, stabilise=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, self.STAB_WANT):
            out += self._stabilised_of(slot, rows)
        return out

    # temporal denoising
    DEN_WANT = ('den', 'den_stats')

    @staticmethod
    def _denoised_of(slot, rows):
        """The rows of a finished denoising replay as Denoised tuples (copies)."""
        d, s = (getattr(slot, name).numpy() for name in FlowEstimator.DEN_WANT)
        return [Denoised(d[i, :h, :w].copy(), int(s[i, 1]), int(s[i, 0]),
                         dict(eligible=int(s[i, 2]), fresh=int(s[i, 3]), rejected=int(s[i, 4]), history=int(s[i, 5]) / float(h * w)))
                for i, h, w in rows]

    def push_denoised(self, frames):
        """push's frames on an estimator built with denoise: one Denoised(frame, noise, tol, counts) per new pair (the count is
        push's).  For the pair (n, n + 1): frame, frame n + 1 averaged with the history of the clip up to frame n, fetched along
        the pair's backward flow — four taps at 1/64 px, 8.8 colours; noise, the pair's noise level M; tol, the tolerance it was
        filtered with; counts, dict(eligible, fresh, rejected, history): the pixels that had a history, those that started a new
        one (no usable flow, a source outside the frame, or occluded in frame n), those whose history was dropped because it was
        too far from the frame, and the mean history count behind the pair.  The clip's first frame is its own denoised frame
        and is not returned.  Bit-reproducible from run to run.  reset() starts a new history."""
        self._mode('push_denoised', sequence=True, denoise=True)
        return self._denoised_of(*self._push(frames, self.DEN_WANT))

    def denoise_sequence(self, frames):
        """Temporal denoising along a clip: T >= 2 frames -> T - 1 Denoised tuples (push_denoised's), of frames 1 .. T - 1."""
        self._mode('denoise_sequence', sequence=True, denoise=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, self.DEN_WANT):
            out += self._denoised_of(slot, rows)
        return out

    # held-out scores of the in-between frames
    HELD_WANT = ('mid', 'mid_holes', 'mid_sse', 'mid_ssim')

    @staticmethod
    def _held_out_of(slot, rows):
        """The rows of a finished held-out replay as HeldOut tuples (copies)."""
        sse, ssim = slot.mid_sse.numpy(), slot.mid_ssim.numpy()
        out = []
        for (i, h, w), m in zip(rows, FlowEstimator._interpolated_of(slot, rows)):
            e = sse[:, i].astype(np.int64)
            out.append(HeldOut(m.frames, m.holes, e, mid_psnr(e, 3 * h * w), mid_mean_ssim(ssim[:, i], mid_windows(h, w))))
        return out

    def push_held_out(self, frames, truths):
        """push_interpolated's frames on an estimator built with held_out=True, with the frames that were left out of the clip:
        truths[i] holds the n frames between the frame before frames[i] and it — a sequence of n [h, w, 3] arrays or one [n, h, w,
        3], of the clip's size and dtype, host arrays or tensors of this device; None only for a clip's first frame.  Returns one
        HeldOut(frames, holes, sse, psnr, ssim) per new pair (the count is push's): push_interpolated's frames and holes, and per
        in-between frame j and kind (MID_KINDS: the interpolated frame, the temporal blend, the nearest frame) sse int64 [n, 3],
        psnr [n, 3] = 10 log10(255^2 3 h w / sse) (inf at sse = 0) and ssim [n, 3], the mean SSIM over the 8 x 8 windows inside the
        frame and the channels (nan without a window)."""
        self._mode('push_held_out', sequence=True, interpolate=True, held_out=True)
        slot = self._submit_sequence(list(frames), self.HELD_WANT, truths=list(truths))
        slot.wait()
        return self._held_out_of(slot, slot.pending[0])

    def evaluate_interpolation(self, clips, num=None):
        """The held-out protocol over full-rate clips: `clips` yields lists of frames; of each, frames 0, n + 1, 2 (n + 1), ... go
        to the network, the n frames between two of them are the truths of that pair, and trailing frames that complete no pair
        are dropped.  reset() between clips.  num: at most that many pairs.  Returns psnr/<kind> and ssim/<kind> for the kinds mid,
        blend, nearest — PSNR from the summed integer squared errors (the pooled MSE), SSIM from the summed window sums and counts
        — the same per position j as psnr_j/<kind> and ssim_j/<kind> (lists of n), holes (the share of interpolated pixels that no
        source reached) and holes_j, num_examples, per_clip (the pairs of every clip) and per_frame: per pair a dict(sse, psnr,
        ssim, holes, shape), so that a mean of per-frame PSNRs can be formed by the caller."""
        self._mode('evaluate_interpolation', sequence=True, interpolate=True, held_out=True)
        n = self.interpolate
        sse, ssim = np.zeros((n, 3), np.int64), np.zeros((n, 3))
        values = wins = 0
        holes = np.zeros(n, np.int64)
        per_clip, per_frame = [], []
        for clip in clips:
            if num is not None and len(per_frame) >= int(num):
                break
            clip = list(clip)
            pairs = (len(clip) - 1) // (n + 1)
            if pairs < 1:
                raise ValueError("evaluate_interpolation: a clip of %d frames holds no pair with %d held-out frame(s)" % (len(clip), n))
            net = clip[:pairs * (n + 1) + 1:n + 1]
            truths = [None] + [clip[p * (n + 1) + 1:(p + 1) * (n + 1)] for p in range(pairs)]
            n0 = len(per_frame)
            for slot, rows, _ in self._pipeline_sequence(net, self.HELD_WANT, truths=truths):
                raw = slot.mid_ssim.numpy()
                for (i, h, w), sc in zip(rows, self._held_out_of(slot, rows)):
                    if num is not None and len(per_frame) >= int(num):
                        break
                    sse += sc.sse
                    ssim += raw[:, i]
                    values += 3 * h * w
                    wins += mid_windows(h, w)
                    holes += sc.holes
                    per_frame.append(dict(sse=sc.sse, psnr=sc.psnr, ssim=sc.ssim, holes=sc.holes, shape=(h, w)))
            per_clip.append(len(per_frame) - n0)
        if not per_frame:
            raise ValueError("evaluate_interpolation: the input yielded no pairs")
        out = {}
        for k, kind in enumerate(MID_KINDS):
            out['psnr/' + kind] = float(mid_psnr(sse[:, k].sum(), n * values))
            out['ssim/' + kind] = float(mid_mean_ssim(math.fsum(ssim[:, k]), n * wins))
            out['psnr_j/' + kind] = [float(v) for v in mid_psnr(sse[:, k], values)]
            out['ssim_j/' + kind] = [float(v) for v in mid_mean_ssim(ssim[:, k], wins)]
        out.update(holes=float(holes.sum()) / (n * values // 3), holes_j=[float(v) / (values // 3) for v in holes],
                   num_examples=len(per_frame), per_clip=per_clip, per_frame=per_frame, sse=sse)
        return out

    # ground truth along a clip
    def _scored_want(self):
        """What a scored replay copies back besides the scores themselves (sums and counts come with nmaps)."""
        want = ('flow',) + (('occ_counts',) if self.seq_bidir else ())
        if self.track:
            want += ('track_scores', 'track_err', 'gt_track_disp', 'gt_track_alive')
        return want

    def _scores_of(self, slot, rows, nmaps):
        """The rows of a finished scored replay as PairScore tuples (copies)."""
        sums, counts = slot.sums.numpy(), slot.counts.numpy()
        out = []
        for (i, h, w), flow in zip(rows, self._flows_of(slot, rows)):
            msum = [float(sums[i, m, 1]) for m in range(nmaps)]
            aee = [float(sums[i, m, 0]) / msum[m] if msum[m] else float('nan') for m in range(nmaps)]
            outl = [100.0 * float(counts[i, m]) / msum[m] if msum[m] else float('nan') for m in range(nmaps)]
            occ = [int(v) for v in slot.occ_counts.numpy()[i]] if self.seq_bidir and nmaps == 2 else None
            track = None
            if self.track:
                shape = self._track_shape(h, w)
                n = int(np.prod(shape))
                track = track_score(slot.track_scores.numpy()[i], float(slot.track_err.numpy()[i]),
                                    slot.gt_track_disp.numpy()[i, :n].reshape(shape + (2,)).copy(),
                                    slot.gt_track_alive.numpy()[i, :n].reshape(shape).astype(bool))
            out.append(PairScore(flow, aee, outl, msum, occ, track))
        return out

    def push_scored(self, frames, gts):
        """push's frames on an estimator built with ground_truth=True, with the ground truth of the pairs they end: gts[i] is
        that of the pair ending at frames[i] — (flow [h, w, 2], mask [h, w] or [h, w, 1]), or the two-map (flow_occ, mask_occ,
        flow_noc, mask_noc) — at the frames' own size, host arrays or tensors of this device; None only for a clip's first
        frame.  One map count per clip.  Returns one PairScore(flow, aee, outliers, mask_sum, occ_counts, track) per new pair
        (the count is push's): aee and outliers (%) per map as evaluate forms them, occ_counts [tp, fp, fn] on a
        sequence='bidirectional' estimator with two maps (else None), track a TrackScore on an estimator with track (else
        None): the tracks of push_tracks against the chained ground-truth flow, ended at its invalid (two maps: or occluded)
        pixels."""
        self._mode('push_scored', sequence=True, ground_truth=True)
        slot = self._submit_sequence(list(frames), self._scored_want(), gts=list(gts))
        slot.wait()
        return self._scores_of(slot, *slot.pending)

    def evaluate_sequence(self, clips, num=None):
        """Scores along clips: `clips` yields (frames, gts) per clip, gts[i] the ground truth (push_scored's forms) of the pair
        (frames[i], frames[i + 1]), len(gts) == len(frames) - 1.  reset() between clips; every frame is uploaded and encoded
        once.  num: at most that many pairs.  Returns evaluate's dictionary — the per-pair averages of AEE/<map> and
        outliers/<map>, num_examples, per_example, names; with both directions and two maps the pooled occ/precision, occ/recall,
        occ/F1 and occ_counts — and per_clip, the number of pairs of every clip.  With track also track/epe, track/delta_avg (the
        mean of pos_acc), track/AJ (the mean of jaccard) and track/occ_acc, pooled over all pairs from the summed integer words,
        and per_example_track (the TrackScore of every pair, without its arrays)."""
        self._mode('evaluate_sequence', sequence=True, ground_truth=True)
        names, rows, occ_rows, per_clip, tracks = None, [], [], [], []
        words, err = np.zeros(16, np.int64), 0.0
        for frames, gts in clips:
            if num is not None and len(rows) >= int(num):
                break
            frames, gts = list(frames), list(gts)
            if len(gts) != len(frames) - 1:
                raise ValueError("evaluate_sequence: a clip of %d frames has %d pairs, got %d ground truths"
                                 % (len(frames), max(len(frames) - 1, 0), len(gts)))
            n0 = len(rows)
            for slot, pairs, nmaps in self._pipeline_sequence(frames, self._scored_want(), gts=[None] + gts):
                for i, sc in zip((p[0] for p in pairs), self._scores_of(slot, pairs, nmaps)):
                    if num is not None and len(rows) >= int(num):
                        break
                    if names is None:
                        names = [n for m in MAP_NAMES[nmaps] for n in ('AEE/' + m, 'outliers/' + m)]
                    elif len(names) != 2 * nmaps:
                        raise ValueError("evaluate_sequence: the clips' ground truth changed its number of maps")
                    rows.append([v for m in range(nmaps) for v in (sc.aee[m], sc.outliers[m])])
                    if sc.occ_counts is not None:
                        occ_rows.append(sc.occ_counts)
                    if sc.track is not None:
                        tracks.append(sc.track._replace(gt_disp=None, gt_alive=None))
                        words += slot.track_scores.numpy()[i].astype(np.int64)
                        err += float(slot.track_err.numpy()[i])
            per_clip.append(len(rows) - n0)
        if not rows:
            raise ValueError("evaluate_sequence: the input yielded no pairs")
        avg = np.mean(np.asarray(rows, dtype=np.float64), axis=0)
        out = {k: float(v) for k, v in zip(names, avg)}
        out.update(num_examples=len(rows), per_example=rows, names=names, per_clip=per_clip)
        if occ_rows and len(occ_rows) == len(rows):
            out.update(occlusion_scores(occ_rows))
            out['occ_counts'] = occ_rows
        if tracks:
            pooled = track_score(words, err, None, None)
            out.update({'track/epe': pooled.epe, 'track/delta_avg': float(np.mean(pooled.pos_acc)),
                        'track/AJ': float(np.mean(pooled.jaccard)), 'track/occ_acc': pooled.occ_acc,
                        'per_example_track': tracks})
        return out

    def _pipeline_sequence(self, frames, want, files=None, max_flow=None, gts=None, truths=None):
        """reset, then _one_ahead over pushes of B frames (gts: the ground truth per frame, chunked alongside; truths: the held-out
        frames per frame, likewise)."""
        self.reset()

        def replays():
            total = 0
            for chunk in chunks(frames, self.B):
                total += len(chunk)
                if truths is not None:
                    yield self._submit_sequence(chunk, want, files, max_flow, truths=truths[total - len(chunk):total])
                    continue
                if gts is not None:
                    yield self._submit_sequence(chunk, want, files, max_flow, gts=gts[total - len(chunk):total])
                    continue
                yield self._submit_sequence(chunk, want, files, max_flow)
            if total < 2:                         # raised before the only replay, which holds no pair, would be handed out
                raise ValueError("a clip needs at least two frames, got %d" % total)
        yield from self._one_ahead(replays())

    def estimate_sequence(self, frames):
        """Flow along a clip: frames = T >= 2 frames (a list or an iterator; [h, w, 3] uint8 or float32 in [0, 255], one size)
        -> T - 1 flows [h, w, 2] float32, frame n -> frame n + 1."""
        self._mode('estimate_sequence', sequence=True)
        out = []
        for slot, rows, _ in self._pipeline_sequence(frames, ('flow',)):
            out += self._flows_of(slot, rows)
        return out

    def export_sequence(self, frames, out_dir, fmt='png', workers=0, level=6, deflate='host', backward=False, occlusion=False,
                        visual=False, max_flow=None, tracks=False, interpolate=False, stabilise=False, denoise=False):
        """estimate_sequence's flows as files: out_dir/%06d_10.png (KITTI 16-bit RGB) or out_dir/%06d_10.flo for pair n (frame n
        -> frame n + 1), with export's writers.  Returns the written paths.  workers, level: as for export (0: the host
        writers; >= 1: the row filters on the device and a writer pool; the captured graph is the same one).  deflate: as for
        export ('device': unflow_deflate behind the filter launch; needs workers >= 1).
        backward: also the backward flow (frame n + 1 -> frame n), %06d_01.png / .flo; occlusion: the forward occlusion mask,
        %06d_10_occ.png (8-bit grey, 255 = occluded) — export's files, per pair in export's order (_10, _01, _10_occ).  Both need
        an estimator built with sequence='bidirectional'.
        visual (an estimator built with visual='sequence'): after those, per pair, the 8-bit pictures of push_visual —
        sequence_visual_files' %06d_img.png (overlay), %06d_flow.png (flow colours), %06d_diff.png (brightness error) and, on a
        sequence='bidirectional' estimator, %06d_flow_bw.png (the backward flow's colours) and %06d_diff_noc.png (the brightness
        error of the non-occluded pixels); max_flow: the scale of the flow colours for the whole clip (None: per pair).
        tracks (an estimator built with track): the tracks of push_tracks.  Dense: after a pair's other files %06d_track.flo,
        the displacement from frame 0 to frame n + 1 on the gh x gw anchor grid, a dead track written as (1e10, 1e10) — the
        .flo unknown-flow value, read back as mask = 0 — through the same writer as the other .flo files.  Sparse anchors: one
        tracks.npz behind the last pair's files, with anchors [N, 2] int32, disp [T - 1, N, 2] float32, alive [T - 1, N] bool.
        interpolate (an estimator built with interpolate=n): the in-between frames of push_interpolated, %06d_mid%d.png (pair, j =
        1..n), 8-bit RGB, behind a pair's pictures — through either writer, the same pixels.
        stabilise (an estimator built with stabilise): behind a pair's other files %06d_stab.png, the stabilised frame of
        push_stabilised (8-bit RGB), and %06d_motion.png, its residual map (8-bit grey, quarter pixels) — through any writer, the
        same pixels; behind the last pair's files one camera.npz with motion [T - 1, 8], path [T - 1, 8], counts [T - 1, 4] and
        matrix [T - 1, 2, 3], camera_matrix of every pair's motion.
        denoise (an estimator built with denoise): behind everything else of a pair %06d_den.png, the denoised frame of
        push_denoised (8-bit RGB; pair n's is frame n + 1) — through any writer, the same pixels.  The clip's first frame is its
        own denoised frame and is not written."""
        from .png_device import check_deflate_mode
        self._mode('export_sequence', sequence=True)
        if tracks and not self.track:
            raise ValueError("export_sequence: the tracks need FlowEstimator(..., sequence=%r, track=True) (or track=S, or "
                             "track=anchors)" % ('bidirectional' if self.seq_bidir else True))
        on_device = check_deflate_mode(deflate, workers)
        if fmt not in ('png', 'flo'):
            raise ValueError("export_sequence: fmt must be 'png' or 'flo'")
        if (backward or occlusion) and not self.seq_bidir:
            raise ValueError("export_sequence: backward / occlusion files need FlowEstimator(..., sequence='bidirectional')")
        if visual and not self.visual:
            raise ValueError("export_sequence: the pictures need %s" % self._visual_spelling())
        if interpolate and not self.interpolate:
            raise ValueError("export_sequence: the in-between frames need FlowEstimator(..., sequence=%r, interpolate=n)"
                             % ('bidirectional' if self.seq_bidir else True))
        if stabilise and not self.stabilise:
            raise ValueError("export_sequence: the stabilised frames need FlowEstimator(..., sequence=%r, stabilise=True)"
                             % ('bidirectional' if self.seq_bidir else True))
        if denoise and not self.denoise:
            raise ValueError("export_sequence: the denoised frames need FlowEstimator(..., sequence='bidirectional', denoise=True)")
        if max_flow is not None and not visual:
            raise ValueError("export_sequence: max_flow scales the flow colours of the pictures; it needs visual=True")

        def plan(n, nmaps):
            return pair_files(n, fmt, backward, occlusion, sequence_visual_files(n, self.seq_bidir) if visual else (),
                              track=dense, mid=self.interpolate if interpolate else 0, stab=bool(stabilise),
                              den=bool(denoise))
        dense = bool(tracks) and self.track_spec[0] == 'dense'
        sparse = [] if tracks and not dense else None      # sparse anchors: the Track of every pair, for tracks.npz
        camera = [] if stabilise else None                 # (motion, path, counts, matrix) of every pair, for camera.npz

        def replays(want, files):
            if sparse is not None:
                want += ('track_disp', 'track_alive')
            if camera is not None:
                want += tuple(n for n in self.STAB_WANT[2:] if n not in want)
            for slot, rows, nmaps in self._pipeline_sequence(frames, want, files, max_flow):
                if sparse is not None:
                    sparse.extend(self._tracks_of(slot, rows))
                if camera is not None:
                    camera.extend((slot.stab_motion.numpy()[i].copy(), slot.stab_path.numpy()[i].copy(),
                                   slot.stab_counts.numpy()[i].astype(np.int64), camera_matrix(slot.stab_motion.numpy()[i], h, w))
                                  for i, h, w in rows)
                yield slot, rows, nmaps
        paths = self._write_files(replays, plan, out_dir, workers, level, on_device)
        if sparse is not None:
            paths.append(os.path.join(out_dir, 'tracks.npz'))
            np.savez(paths[-1], anchors=self.track_spec[1], disp=np.stack([t.disp for t in sparse]),
                     alive=np.stack([t.alive for t in sparse]))
        if camera is not None:
            paths.append(os.path.join(out_dir, 'camera.npz'))
            np.savez(paths[-1], **{k: np.stack([c[j] for c in camera]) for j, k in enumerate(('motion', 'path', 'counts', 'matrix'))})
        return paths
