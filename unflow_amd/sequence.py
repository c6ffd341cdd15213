"""python -m unflow_amd.sequence: the flow along a clip of frames with a trained experiment — every frame uploaded and encoded
once (core/inference.FlowEstimator(..., sequence=True)).

    python -m unflow_amd.sequence --ex NAME --frames DIR [--out DIR] [--flo] [--batch B] [--net_size H W] [--host_decode]
                                  [--output_backward] [--occlusion] [--visual] [--max_flow F]
                                  [--track] [--track_stride S] [--track_points FILE] [--interpolate N [--order K] [--held_out]]
                                  [--stabilise [--stabilise_tol K] [--stabilise_iters R] [--stabilise_follow S]]
                                  [--denoise [--denoise_tol {auto,0..4}] [--denoise_depth D]]

The frames are the 8-bit RGB PNG files of DIR in sorted order, all of one size; pair n is (frame n, frame n + 1).  They are
inflated by a thread pool and decoded on the device, one launch per replay's frames (--host_decode: the host decoder).  The
experiment's config and latest checkpoint are found as python -m unflow_amd.evaluate finds them.  Files go to <--out>/NAME/:
%06d_10.png (KITTI 16-bit flow) or, with --flo, %06d_10.flo — with --workers N (N >= 1) through the device encode path (--level L);
the default and --host_encode: the host's writers.  --output_backward adds the backward flow of every pair (%06d_01.png / .flo),
--occlusion its forward occlusion mask (%06d_10_occ.png); either one runs both directions along the clip
(FlowEstimator(..., sequence='bidirectional')).  --visual adds the pictures of every pair: %06d_img.png,
%06d_flow.png, %06d_diff.png and, where both directions run, %06d_flow_bw.png and %06d_diff_noc.png; --max_flow F colours the
whole clip with one scale instead of every pair with its own maximum.  --track follows every pixel of the first frame along the
clip and adds %06d_track.flo per pair: the displacement from frame 0 to frame n + 1, (1e10, 1e10) where the track
has left the frame or — where both directions run — was occluded; --track_stride S: every S-th pixel of every S-th row instead;
--track_points FILE: the pixels listed in FILE, `x y` per line, written as one tracks.npz (anchors, disp, alive).
--interpolate N (1..7) adds N in-between frames per pair, %06d_mid%d.png (pair, j = 1..N): frame j is at time
j / (N + 1) between the pair's frames, motion-compensated along the flow (along both flows, occluded pixels unblended, where both
directions run).  --order K (1..4, with --interpolate N) orders that splat: every pixel is weighted by how well the
two frames agree along its flow, the weight halving per 64 >> K summed grey levels, pixels that disagree are not blended, and in
one direction a hole takes the later frame's colour; the files are the same.  --held_out (with --interpolate N) scores them: DIR is then the FULL-RATE clip, frames 0, N + 1,
2 (N + 1), ... go to the network, the N frames between two of them are held out, and trailing frames that complete no pair are
dropped (their number is printed).  It prints PSNR and SSIM of the interpolated frames, of the temporal blend and of the nearest
frame against the held-out frames, over the clip and per position j, and the share of hole pixels; the files are then those of the
subsampled clip, pairs numbered along it.
--stabilise fits the camera motion of every pair and adds %06d_stab.png, frame n + 1 resampled along the camera path
(black where the path leaves the frame), %06d_motion.png, every pixel's distance from the pair's dominant motion in quarter pixels
(the independently moving objects), and one camera.npz (motion, path, counts, matrix per pair).  --stabilise_tol K (0..4, default
2): the weight of a pixel halves per 2^(1 - K) px of residual; --stabilise_iters R (0..4, default 3): reweighted fits behind the
first; --stabilise_follow S (0..8, default 0 = lock on the first frame): the path loses 2^-S of its offset per pair.
--denoise (with --output_backward or --occlusion: it needs both directions along the clip) adds %06d_den.png per pair (DESIGN
7.21): frame n + 1 averaged with its own history, fetched along the backward flow; the clip's first frame is its own denoised
frame and is not written.  --denoise_tol (auto, the default, or 0..4): the distance between a pixel and its history that halves the
history's weight is 8 * 2^tol grey levels, auto chooses it per pair from the pair's noise level; --denoise_depth D (1..64, default
8): the longest average."""
import argparse
import os
import sys


def read_frame(path):
    """One 8-bit RGB PNG as uint8 [h, w, 3] (the project's own decoder); anything else: ValueError naming the file."""
    import numpy as np
    from .core.input import decode_png
    try:
        with open(path, 'rb') as f:
            a = decode_png(f.read())
    except Exception as err:                      # a broken file: say which one
        raise ValueError("%s: not a readable PNG (%s)" % (path, err))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("%s: not an 8-bit RGB PNG (%s %s)" % (path, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def _inflate_frame(path):
    """Worker: one 8-bit RGB PNG file -> its inflated scanlines (png_scanlines); read_frame's messages for anything else."""
    import numpy as np
    from .core.png_device import _CHANNELS, _check_variant, _walk_chunks, png_scanlines
    try:
        with open(path, 'rb') as f:
            data = f.read()
        w, h, depth, ctype, _, _, interlace = _walk_chunks(data)[0]
        _check_variant(depth, ctype, interlace)
    except Exception as err:
        raise ValueError("%s: not a readable PNG (%s)" % (path, err))
    if depth != 8 or ctype != 2:                  # from the IHDR: a wrong file is refused before it is inflated
        raise ValueError("%s: not an 8-bit RGB PNG (%s %s)" % (path, np.dtype('uint%d' % depth), (h, w, _CHANNELS[ctype])))
    try:
        return png_scanlines(data)
    except Exception as err:
        raise ValueError("%s: not a readable PNG (%s)" % (path, err))


def device_frames(files, batch, device=None, workers=8):
    """The frames of a clip as uint8 [h, w, 3] DEVICE tensors, equal to read_frame's arrays: a thread pool inflates the files,
    unflow_png_unfilter decodes `batch` frames — one replay's — per launch on the current stream, and the next replay's files
    inflate meanwhile.  A broken or non-8-bit-RGB file raises read_frame's ValueError when its group is reached."""
    from concurrent.futures import ThreadPoolExecutor
    from .core.png_device import MAX_WORKERS, decode_scanlines_device
    groups = [files[i:i + batch] for i in range(0, len(files), batch)]
    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)), thread_name_prefix="png-inflate") as pool:
        ahead = [pool.submit(_inflate_frame, p) for p in groups[0]] if groups else []
        for k in range(len(groups)):
            cur, ahead = ahead, ([pool.submit(_inflate_frame, p) for p in groups[k + 1]] if k + 1 < len(groups) else [])
            try:
                scans = [f.result() for f in cur]
            except BaseException:
                for f in ahead:
                    f.cancel()
                raise
            yield from decode_scanlines_device(scans, device)


def frame_files(folder):
    return [os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.lower().endswith('.png')]


def png_size(path):
    """(h, w) from a PNG's IHDR, without decoding it."""
    import struct
    with open(path, 'rb') as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError("%s: not a PNG file" % path)
    w, h = struct.unpack('>II', head[16:24])
    return h, w


def read_points(path):
    """The anchors of --track_points: a text file with `x y` per line (integers; blank lines and lines that start with # are
    skipped) -> int32 [N, 2]; anything else: ValueError naming the file and the line."""
    import numpy as np
    pts = []
    try:
        with open(path) as f:
            lines = f.read().splitlines()
    except (OSError, UnicodeDecodeError) as err:
        raise ValueError("%s: not a readable text file (%s)" % (path, err))
    for k, line in enumerate(lines, 1):
        t = line.split()
        if not t or t[0].startswith('#'):
            continue
        try:
            x, y = (int(v) for v in t)
        except ValueError:
            raise ValueError("%s:%d: expected two integers `x y`, got %r" % (path, k, line))
        if not (-2 ** 31 <= x < 2 ** 31 and -2 ** 31 <= y < 2 ** 31):
            raise ValueError("%s:%d: a pixel coordinate outside int32: %r" % (path, k, line))
        pts.append((x, y))
    if not pts:
        raise ValueError("%s: no points" % path)
    return np.asarray(pts, dtype=np.int32)


def parser():
    ap = argparse.ArgumentParser(prog='python -m unflow_amd.sequence', description=__doc__.split('\n')[0])
    ap.add_argument('--ex', required=True, help='experiment name')
    ap.add_argument('--frames', required=True, metavar='DIR', help='folder of 8-bit RGB PNG frames (sorted order)')
    ap.add_argument('--out', default='../out', metavar='DIR', help='output root: files go to <out>/<ex>/')
    ap.add_argument('--flo', action='store_true', help='write %%06d_10.flo (default: KITTI 16-bit %%06d_10.png)')
    ap.add_argument('--batch', type=int, default=4, metavar='B', help='new frames per graph replay')
    ap.add_argument('--net_size', type=int, nargs=2, default=(384, 1280), metavar=('H', 'W'),
                    help='network input size (multiples of 64)')
    ap.add_argument('--output_backward', action='store_true',
                    help='also the backward flow of every pair (frame n + 1 -> frame n): %%06d_01.png / .flo')
    ap.add_argument('--occlusion', action='store_true',
                    help='also the forward-backward occlusion mask of every pair: %%06d_10_occ.png (255 = occluded)')
    ap.add_argument('--visual', action='store_true',
                    help='also the pictures of every pair: %%06d_img.png (overlay), %%06d_flow.png (flow colours), %%06d_diff.png '
                         '(brightness error); with --output_backward or --occlusion also %%06d_flow_bw.png and %%06d_diff_noc.png')
    ap.add_argument('--max_flow', type=float, default=None, metavar='F',
                    help='with --visual: one scale of the flow colours for the whole clip (default: every pair its own maximum)')
    ap.add_argument('--track', action='store_true',
                    help='also follow every pixel of the first frame along the clip: %%06d_track.flo per pair, the displacement '
                         'from frame 0 to frame n + 1, (1e10, 1e10) where the track is dead')
    ap.add_argument('--track_stride', type=int, default=None, metavar='S',
                    help='like --track, for every S-th pixel of every S-th row (files of ceil(h / S) x ceil(w / S) pixels)')
    ap.add_argument('--track_points', default=None, metavar='FILE',
                    help='follow the pixels listed in FILE (`x y` per line) instead: one tracks.npz with anchors, disp and alive')
    ap.add_argument('--interpolate', type=int, default=None, metavar='N',
                    help='also N in-between frames per pair (1..7), motion-compensated: %%06d_mid%%d.png (pair, j = 1..N)')
    ap.add_argument('--order', type=int, default=None, metavar='K',
                    help='with --interpolate N: the consistency-ordered splat of steepness K (1..4) in place of the plain one')
    ap.add_argument('--held_out', action='store_true',
                    help='with --interpolate N: DIR is the full-rate clip; every (N + 1)-th frame goes to the network and the '
                         'in-between frames are scored against the frames left out (PSNR, SSIM; also blend and nearest frame)')
    ap.add_argument('--stabilise', action='store_true',
                    help='also the camera motion of every pair: %%06d_stab.png (frame n + 1 along the camera path), %%06d_motion.png '
                         '(the residual against the dominant motion, quarter pixels) and camera.npz')
    ap.add_argument('--stabilise_tol', type=int, default=None, metavar='K',
                    help='with --stabilise: the weight of a pixel halves per 2^(1 - K) px of residual (0..4, default 2)')
    ap.add_argument('--stabilise_iters', type=int, default=None, metavar='R',
                    help='with --stabilise: reweighted fits behind the first (0..4, default 3)')
    ap.add_argument('--stabilise_follow', type=int, default=None, metavar='S',
                    help='with --stabilise: the path loses 2^-S of its offset per pair (1..8); 0, the default, locks on the first frame')
    ap.add_argument('--denoise', action='store_true',
                    help='also %%06d_den.png per pair: frame n + 1 averaged with its history along the backward flow; needs both '
                         'directions along the clip (--output_backward or --occlusion)')
    ap.add_argument('--denoise_tol', default=None, metavar='{auto,0..4}',
                    help="with --denoise: 8 * 2^tol grey levels between a pixel and its history halve the history's weight; auto "
                         "(the default): per pair, from its noise level")
    ap.add_argument('--denoise_depth', type=int, default=None, metavar='D',
                    help='with --denoise: the longest average, in frames (1..64, default 8)')
    ap.add_argument('--config', default='../config.ini', help='the project config.ini (dirs: log, checkpoints)')
    ap.add_argument('--host_decode', action='store_true', help="decode the frames with the host's PNG decoder (slow)")
    from .evaluate import add_encode_flags
    add_encode_flags(ap)
    return ap


def parse_args(argv=None):
    """Parsed flags plus a.files; a folder that holds no clip is an argparse error (SystemExit, status 2)."""
    ap = parser()
    a = ap.parse_args(argv)
    from .evaluate import check_encode_flags
    check_encode_flags(ap, a)
    if a.batch <= 0:
        ap.error("--batch must be positive")
    if a.max_flow is not None and not a.visual:
        ap.error("--max_flow scales the flow colours of the pictures: it needs --visual")
    if a.max_flow is not None and not a.max_flow > 0:
        ap.error("--max_flow must be positive")
    if a.interpolate is not None and not 1 <= a.interpolate <= 7:
        ap.error("--interpolate makes 1 to 7 in-between frames per pair")
    if a.order is not None and not 1 <= a.order <= 4:
        ap.error("--order is the steepness of the ordered splat, 1 to 4")
    if a.order is not None and a.interpolate is None:
        ap.error("--order orders the splat of the in-between frames: it needs --interpolate N")
    if a.held_out and a.interpolate is None:
        ap.error("--held_out scores the in-between frames: it needs --interpolate N")
    a.stabilise_option = None                     # FlowEstimator's stabilise
    given = {k: getattr(a, 'stabilise_' + k) for k in ('tol', 'iters', 'follow') if getattr(a, 'stabilise_' + k) is not None}
    if given and not a.stabilise:
        ap.error("--stabilise_%s sets the camera-motion fit: it needs --stabilise" % sorted(given)[0])
    if a.stabilise:
        from .core.inference import STABILISE_RANGES
        for k, v in given.items():
            if not STABILISE_RANGES[k][0] <= v <= STABILISE_RANGES[k][1]:
                ap.error("--stabilise_%s is an integer in %d..%d" % ((k,) + STABILISE_RANGES[k]))
        a.stabilise_option = given or True
    a.denoise_option = None                       # FlowEstimator's denoise
    for k in ('tol', 'depth'):
        if getattr(a, 'denoise_' + k) is not None and not a.denoise:
            ap.error("--denoise_%s sets the temporal filter: it needs --denoise" % k)
    if a.denoise:
        if not (a.output_backward or a.occlusion):
            ap.error("--denoise fetches a frame's history along the backward flow: it needs both directions along the clip; add "
                     "--output_backward or --occlusion")
        given = {}
        if a.denoise_tol is not None:
            if a.denoise_tol != 'auto' and a.denoise_tol not in ('0', '1', '2', '3', '4'):
                ap.error("--denoise_tol is auto or an integer in 0..4")
            given['tol'] = a.denoise_tol if a.denoise_tol == 'auto' else int(a.denoise_tol)
        if a.denoise_depth is not None:
            if not 1 <= a.denoise_depth <= 64:
                ap.error("--denoise_depth is an integer in 1..64")
            given['depth'] = a.denoise_depth
        a.denoise_option = given or True
    if a.track_stride is not None and a.track_stride < 1:
        ap.error("--track_stride must be at least 1")
    if a.track_points is not None and (a.track or a.track_stride is not None):
        ap.error("--track_points follows the listed pixels; --track / --track_stride follow a grid: give one or the other")
    a.track_option = False                        # FlowEstimator's track
    if a.track_points is not None:
        try:
            a.track_option = read_points(a.track_points)
        except ValueError as err:
            ap.error("--track_points %s" % err)
    elif a.track or a.track_stride is not None:
        a.track_option = a.track_stride if a.track_stride is not None else True
    if a.net_size[0] % 64 or a.net_size[1] % 64 or min(a.net_size) <= 0:
        ap.error("--net_size: H and W must be positive multiples of 64")
    if not os.path.isdir(a.frames):
        ap.error("--frames %s: not a folder" % a.frames)
    a.files = frame_files(a.frames)
    if len(a.files) < 2:
        ap.error("--frames %s: a clip needs at least two PNG frames, found %d%s"
                 % (a.frames, len(a.files), (" (%s)" % a.files[0]) if a.files else ""))
    try:
        sizes = [png_size(p) for p in a.files]
    except ValueError as err:
        ap.error(str(err))
    for p, s in zip(a.files, sizes):
        if s != sizes[0]:
            ap.error("%s: a %dx%d frame in a clip of %dx%d frames (%s)" % (p, s[0], s[1], sizes[0][0], sizes[0][1], a.files[0]))
    a.frame_size = sizes[0]
    a.full_rate, a.dropped = None, 0
    if a.held_out:                                # the full-rate clip: every (N + 1)-th frame is a network frame
        pairs = (len(a.files) - 1) // (a.interpolate + 1)
        if pairs < 1:
            ap.error("--frames %s: --held_out with --interpolate %d needs at least %d frames, found %d"
                     % (a.frames, a.interpolate, a.interpolate + 2, len(a.files)))
        a.full_rate = a.files[:pairs * (a.interpolate + 1) + 1]
        a.dropped = len(a.files) - len(a.full_rate)
        a.files = a.full_rate[::a.interpolate + 1]
    return a


def held_out_table(scores, n):
    """evaluate_interpolation's dictionary as the lines the command prints: a row per kind, PSNR and SSIM over the clip and per j."""
    from .core.inference import MID_KINDS
    lines = ["%-8s %10s %10s  %s" % ("", "PSNR", "SSIM", "  ".join("j=%d PSNR / SSIM     " % j for j in range(1, n + 1)))]
    for kind in MID_KINDS:
        per_j = "  ".join("%8.4f / %8.6f" % (p, q) for p, q in zip(scores['psnr_j/' + kind], scores['ssim_j/' + kind]))
        lines.append("%-8s %10.4f %10.6f  %s" % (kind, scores['psnr/' + kind], scores['ssim/' + kind], per_j))
    lines.append("holes    %.4f %% of the interpolated pixels (%s)"
                 % (100.0 * scores['holes'], "  ".join("j=%d %.4f %%" % (j + 1, 100.0 * v) for j, v in enumerate(scores['holes_j']))))
    return lines


def main(argv=None):
    a = parse_args(argv)
    from .core.inference import FlowEstimator
    from .core.util import config_dict, convert_input_strings
    from .evaluate import experiment_paths
    cfg_path, ckpt_dir = experiment_paths(a.ex, a.config)
    config = config_dict(cfg_path)
    params = dict(config.get('train', {}))
    convert_input_strings(params, config_dict(a.config).get('dirs', {}))
    params.update(config.get('train_kitti', {}))
    est = FlowEstimator.from_checkpoint(ckpt_dir, params, a.batch, net_size=tuple(a.net_size), max_frame=a.frame_size,
                                        sequence='bidirectional' if (a.output_backward or a.occlusion) else True,
                                        visual='sequence' if a.visual else False, track=a.track_option,
                                        interpolate=a.interpolate, held_out=a.held_out, interpolate_order=a.order,
                                        stabilise=a.stabilise_option, denoise=a.denoise_option)
    out_dir = os.path.join(a.out, a.ex)
    print("-- %s (step %s): %d frames of %dx%d from %s" % (a.ex, est.global_step, len(a.files), a.frame_size[0], a.frame_size[1],
                                                           a.frames))
    try:
        if a.held_out:
            if a.dropped:
                print("dropped %d trailing frame(s) that complete no pair of %d held-out frame(s)" % (a.dropped, a.interpolate))
            full = [read_frame(p) for p in a.full_rate] if a.host_decode else list(device_frames(a.full_rate, a.batch, est.dev))
            scores = est.evaluate_interpolation([full])
            print("held out: %d pair(s), %d frame(s) each" % (scores['num_examples'], a.interpolate))
            print("\n".join(held_out_table(scores, a.interpolate)))
            del full
        frames = (read_frame(p) for p in a.files) if a.host_decode else device_frames(a.files, a.batch, est.dev)
        paths = est.export_sequence(frames, out_dir, fmt='flo' if a.flo else 'png', workers=a.encode_workers, level=a.level,
                                    deflate=a.deflate, backward=a.output_backward, occlusion=a.occlusion, visual=a.visual,
                                    max_flow=a.max_flow, tracks=a.track_option is not False,
                                    interpolate=a.interpolate is not None, stabilise=a.stabilise,
                                    denoise=a.denoise)
    except ValueError as err:
        raise SystemExit("Error: %s" % err)
    print("wrote %d files to %s" % (len(paths), out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
