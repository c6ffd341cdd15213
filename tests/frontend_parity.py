"""Shapes, deterministic inputs, fp64 / fp32 references, comparators and torch stand-ins (with named mutants) of the per-element
parity tests of the kernels at the two ENDS of the pipeline (tests/test_frontend_kernels_gpu.py, proven without a GPU by
tests/test_frontend_parity_cpu.py): unflow_stn_affine_fwd and unflow_photometric_augment (csrc/augment.hip),
unflow_inference_input / _input_frames / _output / _occlusion (csrc/inference.hip).  Not a test file.

References call oracle/model_ref.py and numpy only (M.stn_transformer, M.random_photometric_apply, M.resize_bilinear_tf1,
M.image_warp, M.length_sq) — never unflow_amd.core.input, core.losses or the library, whose chains share their expressions with
the kernels under test.  Every input is an fp32 (or uint8) array; the fp64 reference gets it widened, the fp32 evaluation of the
same oracle is the yardstick of what fp32 arithmetic delivers.  The standing bound: an error over the tensor's max of at most
max(floor, 2 x the fp32 oracle's own error).  Exclusions are computed here, in fp64, from the inputs alone, and each has a share
cap.  The `standin_*` functions are fp32 torch transcriptions with switchable faults: the mutants the CPU proof sees rejected."""
import functools

import numpy as np
import torch

import loss_parity as L
from oracle import model_ref as M

F32, F64 = torch.float32, torch.float64
FLOOR = 1e-6
SENTINEL = -777.25
CHANNEL_MEAN = tuple(float(np.float32(v)) for v in M.CHANNEL_MEAN)      # the fp32 values the C ABI carries, on both sides


def _mean(dt):
    return torch.tensor(CHANNEL_MEAN, dtype=F64).to(dt) / 255.0


def frame_region(row, h, w, y0, x0):
    """The (h, w) region at origin (y0, x0) of a staging row [Hmax, Wmax, ...]; zero outside the buffer."""
    Hm, Wm = row.shape[:2]
    out = torch.zeros((h, w) + tuple(row.shape[2:]), dtype=row.dtype)
    r0, r1, c0, c1 = max(y0, 0), min(y0 + h, Hm), max(x0, 0), min(x0 + w, Wm)
    if r1 > r0 and c1 > c0:
        out[r0 - y0:r1 - y0, c0 - x0:c1 - x0] = row[r0:r1, c0:c1]
    return out


def place_region(row, frame, y0, x0):
    """The inverse: write `frame` at origin (y0, x0) of `row`, dropping what falls outside."""
    Hm, Wm = row.shape[:2]
    h, w = frame.shape[:2]
    r0, r1, c0, c1 = max(y0, 0), min(y0 + h, Hm), max(x0, 0), min(x0 + w, Wm)
    if r1 > r0 and c1 > c0:
        row[r0:r1, c0:c1] = frame[r0 - y0:r1 - y0, c0 - x0:c1 - x0]


def desc_rows(frames, u8=False):
    """[B, 8] int32 table written by hand: {h, w, y0, x0, nmaps, u8, 0, 0} (include/unflow_hip.h)."""
    d = np.zeros((len(frames), 8), np.int32)
    for i, f in enumerate(frames):
        d[i, :4] = f[:4]
        d[i, 4] = f[4] if len(f) > 4 else 0
        d[i, 5] = int(u8)
    return d


def check_abs(got, ref, bound, exclude=None, max_share=0.0):
    """max |got - ref| <= bound outside `exclude` (over the leading pixel axes), whose share is capped.  Returns the worst."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    if exclude is not None:
        share = int(exclude.sum()) / exclude.numel()
        assert share <= max_share, ("excluded share", share, max_share)
        err = err.masked_fill(exclude.reshape(exclude.shape + (1,) * (err.dim() - exclude.dim())).expand_as(err), 0.0)
    worst = err.max().item()
    assert worst <= bound, ("abs", worst, bound)            # NaN fails
    return worst


# ================================================================================================ 1. unflow_stn_affine_fwd
# name -> (B, H, W).  BIG: 529,470 px > 2048 * 256 = 524,288: a second grid-stride pass, trailing blocks with nothing to do
STN_SHAPES = {'RAGGED': (3, 19, 45), 'ROW': (2, 7, 70), 'TINY': (2, 2, 3), 'BIG': (3, 333, 530)}
STN_LDS = [(1, 1, 1), (3, 3, 3), (3, 4, 4), (5, 8, 8)]          # (C, ld_u, ld_out): the two specialised templates, the generic one
# (shape, C, ld_u, ld_out, form, thetas, out_size).  form: 'plain' n_u = n_theta = n_out = B; 'mask' n_u = 1, n_theta = B (the border
# mask); 'engine' n_u = 2B, n_theta = B, n_out = 2B (sample n uses theta n % B).  The far thetas need B = 3 (one ordinary sample
# keeps the tensor's max at the image's).
STN_CASES = ([(s, C, lu, lo, 'plain', 'strong', None) for s in ('RAGGED', 'ROW', 'TINY') for C, lu, lo in STN_LDS] + [
    ('RAGGED', 3, 3, 3, 'plain', 'train', None), ('ROW', 3, 3, 3, 'plain', 'train', None), ('TINY', 3, 4, 4, 'plain', 'train', None),
    ('RAGGED', 1, 1, 1, 'plain', 'far', None), ('RAGGED', 3, 3, 3, 'plain', 'far', None), ('RAGGED', 5, 8, 8, 'engine', 'far', None),
    ('RAGGED', 1, 1, 1, 'mask', 'strong', None), ('RAGGED', 1, 1, 1, 'mask', 'train', None), ('TINY', 1, 1, 1, 'mask', 'strong', None),
    ('RAGGED', 3, 3, 3, 'engine', 'strong', None), ('RAGGED', 3, 4, 4, 'engine', 'train', None), ('ROW', 3, 3, 3, 'engine', 'strong', None),
    ('TINY', 5, 8, 8, 'engine', 'strong', None),
    ('RAGGED', 3, 3, 3, 'plain', 'strong', (11, 30)), ('RAGGED', 5, 8, 8, 'plain', 'strong', (40, 64)),
    ('RAGGED', 1, 1, 1, 'mask', 'strong', (40, 64)), ('RAGGED', 3, 3, 3, 'engine', 'train', (11, 30)),
    ('BIG', 1, 1, 1, 'plain', 'strong', None), ('BIG', 3, 3, 3, 'plain', 'strong', None), ('BIG', 3, 4, 4, 'plain', 'train', None),
    ('BIG', 1, 1, 1, 'mask', 'far', None)])
STN_EDGE_MARGIN = 1e-3           # fp64 source coordinate this close to x in {0, W-1} or y in {0, H-1}: the clipped transformer jumps
STN_EDGE_SHARE_CAP = 2e-3


def stn_counts(case):
    """(n_u, n_theta, n_out) of a case."""
    B = STN_SHAPES[case[0]][0]
    return {'plain': (B, B, B), 'mask': (1, B, B), 'engine': (2 * B, B, 2 * B)}[case[4]]


def stn_thetas(kind, B, seed):
    """[B, 6] fp32.  'train': draw_training_augmentation's global transform (flip, scale 0.9 .. 1.1); 'strong': translation
    0.15 / 0.1, rotation 20 deg, scale 0.8 .. 1.2, flip; 'far': one ordinary sample, translation 50 with scale 1e4, translation
    50 with scale 1e9 — floor(x) is past every int there, and both coordinates of every pixel lie outside the image."""
    from unflow_amd.core import augment as A
    g = torch.Generator().manual_seed(seed)
    if kind == 'train':
        th = A.draw_training_augmentation(B, g)['theta_global']
    elif kind == 'strong':
        th = A.draw_affine(B, max_translation_x=0.15, max_translation_y=0.1, max_rotation=20.0, min_scale=0.8, max_scale=1.2,
                           horizontal_flipping=True, generator=g)
    else:
        assert B == 3
        t = torch.tensor
        th = A.affine_theta(t([0.1, 50.0, -50.0]), t([-0.05, -50.0, 50.0]), t([10.0, 0.0, 0.0]), t([0.9, 1e4, 1e9]), t([1.0, 1.0, -1.0]))
    return th.reshape(B, 6).float().contiguous()


def _stn_coords(theta, case):
    """The fp64 source coordinates (x, y), each [n_out, Ho, Wo], of a case under theta [n_theta, 6]."""
    _, H, W = STN_SHAPES[case[0]]
    Ho, Wo = stn_out_size(case)
    _, n_t, n_out = stn_counts(case)
    t = theta.double()[torch.arange(n_out) % n_t].view(n_out, 6, 1, 1)
    xt = (-1.0 + torch.arange(Wo, dtype=F64) * (2.0 / (Wo - 1))).view(1, 1, Wo)
    yt = (-1.0 + torch.arange(Ho, dtype=F64) * (2.0 / (Ho - 1))).view(1, Ho, 1)
    return (t[:, 0] * xt + t[:, 1] * yt + t[:, 2] + 1.0) * W / 2.0, (t[:, 3] * xt + t[:, 4] * yt + t[:, 5] + 1.0) * H / 2.0


def _stn_edge(x, y, H, W):
    m = STN_EDGE_MARGIN
    return (x.abs() < m) | ((x - (W - 1)).abs() < m) | (y.abs() < m) | ((y - (H - 1)).abs() < m)


@functools.lru_cache(maxsize=None)
def make_stn_inputs(case):
    """U [n_u, H, W, C] in [0, 1) and theta [n_theta, 6].  The thetas are redrawn (next seed) until, in fp64, the edge pixels stay
    under their cap and every ordinary sample has a pixel inside the image — at 2 x 3 a draw can put a whole sample outside, or a
    whole row on an edge line (the training ranges have no rotation: a row shares its y)."""
    name, C, _, _, form, kind, _ = case
    B, H, W = STN_SHAPES[name]
    n_u, n_t, _ = stn_counts(case)
    seed = 100 + H + 7 * C + {'plain': 0, 'mask': 1, 'engine': 2}[form]
    U = torch.rand(n_u, H, W, C, generator=torch.Generator().manual_seed(seed))
    for k in range(64):
        theta = stn_thetas(kind, n_t, seed + 1000 + 31 * k)
        x, y = _stn_coords(theta, case)
        inside = ((x > 0) & (x < W - 1) & (y > 0) & (y < H - 1)).flatten(1).any(1)
        if _stn_edge(x, y, H, W).float().mean().item() <= STN_EDGE_SHARE_CAP and bool(inside[:1 if kind == 'far' else None].all()):
            return U, theta
    raise RuntimeError("no admissible theta draw")


def stn_out_size(case):
    _, H, W = STN_SHAPES[case[0]]
    return case[6] or (H, W)


@functools.lru_cache(maxsize=None)
def ref_stn(case, dt):
    U, theta = make_stn_inputs(case)
    n_u, n_t, n_out = stn_counts(case)
    n = torch.arange(n_out)
    return M.stn_transformer(U[n % n_u].to(dt), theta[n % n_t].to(dt).view(-1, 2, 3), case[6])


@functools.lru_cache(maxsize=None)
def stn_pixel_sets(case):
    """From the inputs alone, in fp64: (edge [n_out, Ho, Wo] — the excluded pixels, source coordinate within STN_EDGE_MARGIN of
    the four lines where the clipped transformer is discontinuous; outside — both coordinates at least a pixel past the image:
    both tap pairs collapse and the four terms cancel exactly, in any precision)."""
    _, theta = make_stn_inputs(case)
    _, H, W = STN_SHAPES[case[0]]
    x, y = _stn_coords(theta, case)
    edge = _stn_edge(x, y, H, W)
    outside = ((x <= -2) | (x >= W)) & ((y <= -2) | (y >= H))
    return edge, outside


def standin_stn(U, theta, n_out, out_size=None, mutant=None):
    """spatial_transformer.py written out per output sample, in U's dtype.  Mutants: 'weights_first' (weights formed before the
    indices are clipped), 'step' (linspace step 2 / n), 'nomod' (theta and source indexed by n itself, clamped here), 'halfpix'
    (grid at pixel centres), 'swap_bc' (wb and wc swapped)."""
    dt = U.dtype
    n_u, H, W, C = U.shape
    Ho, Wo = out_size or (H, W)
    n = torch.arange(n_out)
    iu, it = n % n_u, n % theta.shape[0]
    if mutant == 'nomod':
        iu, it = n.clamp(max=n_u - 1), n.clamp(max=theta.shape[0] - 1)
    one = torch.tensor(1.0, dtype=dt)

    def lin(k):
        i = torch.arange(k, dtype=dt) + (0.5 if mutant == 'halfpix' else 0.0)
        return -one + i * ((one - -one) / (k if mutant == 'step' else k - 1))

    x_t = lin(Wo).view(1, 1, Wo).expand(1, Ho, Wo).reshape(1, -1)
    y_t = lin(Ho).view(1, Ho, 1).expand(1, Ho, Wo).reshape(1, -1)
    t = theta.to(dt)[it]
    x = (t[:, 0:1] * x_t + t[:, 1:2] * y_t + t[:, 2:3] + 1.0) * float(W) / 2.0
    y = (t[:, 3:4] * x_t + t[:, 4:5] * y_t + t[:, 5:6] + 1.0) * float(H) / 2.0
    fx, fy = torch.floor(x).long(), torch.floor(y).long()
    x0, x1, y0, y1 = fx.clamp(0, W - 1), (fx + 1).clamp(0, W - 1), fy.clamp(0, H - 1), (fy + 1).clamp(0, H - 1)
    flat = U[iu].reshape(n_out, H * W, C)
    g = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).unsqueeze(-1).expand(-1, -1, C))      # noqa: E731
    Ia, Ib, Ic, Id = g(y0, x0), g(y1, x0), g(y0, x1), g(y1, x1)
    if mutant == 'weights_first':
        x0f, x1f, y0f, y1f = fx.to(dt), (fx + 1).to(dt), fy.to(dt), (fy + 1).to(dt)
    else:
        x0f, x1f, y0f, y1f = x0.to(dt), x1.to(dt), y0.to(dt), y1.to(dt)
    wa, wb = ((x1f - x) * (y1f - y)).unsqueeze(-1), ((x1f - x) * (y - y0f)).unsqueeze(-1)
    wc, wd = ((x - x0f) * (y1f - y)).unsqueeze(-1), ((x - x0f) * (y - y0f)).unsqueeze(-1)
    if mutant == 'swap_bc':
        wb, wc = wc, wb
    return (wa * Ia + wb * Ib + wc * Ic + wd * Id).reshape(n_out, Ho, Wo, C)


def check_stn(got, case):
    """Per element inside max(1e-6, 2 x the fp32 oracle's error) of the tensor's max, the edge pixels excluded (share capped);
    exactly 0 where both coordinates are outside the image.  Returns (worst, the oracle's, bound, edge share, outside share)."""
    got = got.detach().cpu()
    r32, r64 = ref_stn(case, F32), ref_stn(case, F64)
    edge, outside = stn_pixel_sets(case)
    assert bool((r64[outside] == 0).all()), "the fp64 reference is exactly 0 outside the image"
    assert bool((got[outside] == 0).all()), ("not exactly 0 outside the image", int((got[outside] != 0).sum()))
    bound, own = L.grad_bound(r32, r64, edge, floor=FLOOR)
    worst = L.check_grad(got, r64, bound, edge, max_share=STN_EDGE_SHARE_CAP)
    return worst, own, bound, edge.float().mean().item(), outside.float().mean().item()


# ================================================================================================ 2. unflow_photometric_augment
# name -> (N, H, W), N = 2B.  BIG: 705,960 px > 2048 * 256
PHOTO_SHAPES = {'RAGGED': (6, 19, 45), 'ROW': (4, 7, 70), 'TINY': (4, 2, 3), 'BIG': (4, 333, 530)}
PHOTO_FORMS = [(npar, ld_in, ld_out, mean) for npar in ('B', 'N') for ld_in in (3, 4) for ld_out in (3, 4) for mean in (False, True)]
PHOTO_BIG_FORMS = [('B', 4, 4, True), ('N', 3, 3, False)]
PHOTO_ZERO_MARGIN = 1e-5         # fp64 pre-clamp value this close to 0: v^(1/gamma) has unbounded slope there
PHOTO_ZERO_SHARE_CAP = 1e-3
PHOTO_FLOOR = 2e-6               # absolute


def photo_npar(name, code):
    N = PHOTO_SHAPES[name][0]
    return N // 2 if code == 'B' else N


@functools.lru_cache(maxsize=None)
def make_photo_inputs(name):
    """im [N, H, W, 3] in [0, 1] with a block of exact 0 and one of exact 1, and N draws (a case with n_par = B takes the first
    B) over the training ranges widened until both clamps act: contrast +-0.3, brightness +-0.2 (alternating sign, so every batch
    has a sample that clamps low and one that clamps high), colour 0.7 .. 1.3, gamma 0.7 .. 1.5, noise +-0.04."""
    N, H, W = PHOTO_SHAPES[name]
    g = torch.Generator().manual_seed(300 + H)
    u = lambda n, lo, hi: torch.rand(n, generator=g) * (hi - lo) + lo          # noqa: E731
    im = torch.rand(N, H, W, 3, generator=g)
    im[:, 0, :max(W // 4, 1)] = 0.0
    im[:, -1, -max(W // 4, 1):] = 1.0
    sign = torch.tensor([-1.0, 1.0]).repeat(N)[:N]
    draws = dict(contrast=u(N, -0.3, 0.3), brightness=sign * u(N, 0.08, 0.2), colour=u(3 * N, 0.7, 1.3).view(N, 3),
                 gamma=u(N, 0.7, 1.5), noise=u(N, -0.04, 0.04))
    return im, draws


def _photo_draws(name, npar_code, dt):
    im, d = make_photo_inputs(name)
    idx = torch.arange(im.shape[0]) % photo_npar(name, npar_code)
    return im.to(dt), {k: v[idx].to(dt) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def ref_photo(name, npar_code, with_mean, dt):
    im, d = _photo_draws(name, npar_code, dt)
    out = M.random_photometric_apply([im], d['contrast'], d['gamma'], d['colour'], d['noise'], d['brightness'])[0]
    return out - _mean(dt) if with_mean else out


@functools.lru_cache(maxsize=None)
def photo_pixel_sets(name, npar_code):
    """In fp64, from the inputs: (near0 [N, H, W] — a channel's pre-clamp value within PHOTO_ZERO_MARGIN of 0: excluded; the
    shares of values clamped at 0 and at 1)."""
    im, d = _photo_draws(name, npar_code, F64)
    v = lambda t_: t_.view(-1, 1, 1, 1)                                         # noqa: E731
    pre = (im * (v(d['contrast']) + 1.0) + v(d['brightness'])) * d['colour'].view(-1, 1, 1, 3)
    return (pre.abs() < PHOTO_ZERO_MARGIN).any(3), (pre <= 0).double().mean().item(), (pre >= 1).double().mean().item()


def standin_photo(name, npar_code, with_mean, mutant=None):
    """fp32, written out.  Mutants: 'gamma' (gamma where 1 / gamma belongs), 'clamp_after' (clamp after pow), 'colour_idx'
    (colour[s + c]), 'noise_before' (noise added before the clamp), 'mean255' (mean not divided by 255), 'nomod' (s = n)."""
    im, d = make_photo_inputs(name)
    N, n_par = im.shape[0], photo_npar(name, npar_code)
    s = torch.arange(N) % n_par
    if mutant == 'nomod':
        s = torch.arange(N).clamp(max=n_par - 1)
    v = lambda t_: t_[s].view(-1, 1, 1, 1)                                      # noqa: E731
    col = d['colour'][:n_par].reshape(-1)
    ci = (s.view(-1, 1) + torch.arange(3)).clamp(max=col.numel() - 1) if mutant == 'colour_idx' else 3 * s.view(-1, 1) + torch.arange(3)
    r = (im * (v(d['contrast']) + 1.0) + v(d['brightness'])) * col[ci].view(N, 1, 1, 3)
    ex = v(d['gamma']) if mutant == 'gamma' else v(1.0 / d['gamma'])
    if mutant == 'noise_before':
        r = torch.pow(torch.clamp(r + v(d['noise']), 0.0, 1.0), ex)
    elif mutant == 'clamp_after':
        r = torch.clamp(torch.pow(r, ex), 0.0, 1.0) + v(d['noise'])
    else:
        r = torch.pow(torch.clamp(r, 0.0, 1.0), ex) + v(d['noise'])
    if with_mean:
        r = r - (torch.tensor(CHANNEL_MEAN) if mutant == 'mean255' else _mean(F32))
    return r


def check_photo(got, name, npar_code, with_mean):
    """max |got - fp64| <= max(2e-6, 2 x the fp32 oracle's) outside the near-zero pixels.  Returns (worst, oracle's, bound, share)."""
    r32, r64 = ref_photo(name, npar_code, with_mean, F32), ref_photo(name, npar_code, with_mean, F64)
    near0, _, _ = photo_pixel_sets(name, npar_code)
    own = (r32.double() - r64).abs().masked_fill(near0.unsqueeze(3), 0.0).max().item()
    bound = max(PHOTO_FLOOR, 2.0 * own)
    worst = check_abs(got, r64, bound, near0, PHOTO_ZERO_SHARE_CAP)
    return worst, own, bound, near0.float().mean().item()


# ================================================================================================ 3. unflow_inference_input
INPUT_STAGING = (24, 40)
# (h, w, y0, x0): the whole row; inside; off the top; off top, left and right and bottom; off bottom and right; one pixel, one row,
# one column (y1 = min(y0 + 1, h - 1) = y0); an empty slot
INPUT_FRAMES = [(24, 40, 0, 0), (20, 33, 2, 3), (29, 37, -3, 1), (30, 52, -3, -6), (18, 30, 10, 15), (1, 1, 5, 7), (1, 40, 23, 0),
                (24, 1, 0, 39), (0, 0, 0, 0)]
# name -> (frames, (H, W)).  BIG: 2 * 3 * 320 * 320 = 614,400 items > 2048 * 256
INPUT_CASES = {'N16x24': (INPUT_FRAMES, (16, 24)), 'N32x64': (INPUT_FRAMES, (32, 64)),
               'BIG': ([INPUT_FRAMES[1], INPUT_FRAMES[3], INPUT_FRAMES[4]], (320, 320))}


@functools.lru_cache(maxsize=None)
def make_input_case(name, u8):
    """staged [2, B, Hmax, Wmax, 3] (uint8, or fp32 with fractional parts; the empty slot holds data that must not be read) and
    the desc rows."""
    frames, _ = INPUT_CASES[name]
    Hm, Wm = INPUT_STAGING
    rs = np.random.RandomState(11 + len(frames))
    st = rs.randint(0, 256, size=(2, len(frames), Hm, Wm, 3)).astype(np.float32)
    if not u8:
        st = np.minimum(st + rs.rand(*st.shape).astype(np.float32) * 0.75, 255.0).astype(np.float32)
    return (st.astype(np.uint8) if u8 else st), desc_rows(frames, u8)


def oracle_input(row, frame, H, W):
    """One network-input row [H, W, 3] from its staging row [Hmax, Wmax, 3] (already in the dtype to evaluate in)."""
    h, w, y0, x0 = frame[:4]
    if h == 0 or w == 0:
        return torch.zeros(H, W, 3, dtype=row.dtype)
    return M.resize_bilinear_tf1(frame_region(row, h, w, y0, x0).unsqueeze(0), H, W)[0] / 255.0 - _mean(row.dtype)


def _input_rows(name, u8, fn):
    frames, (H, W) = INPUT_CASES[name]
    st, _ = make_input_case(name, u8)
    return torch.stack([fn(st[k, b], frames[b], H, W) for k in range(2) for b in range(len(frames))])


@functools.lru_cache(maxsize=None)
def ref_input(name, u8, dt):
    """[2B, H, W, 3]: rows [0, B) the first frames, [B, 2B) the second."""
    return _input_rows(name, u8, lambda row, f, H, W: oracle_input(torch.from_numpy(row.astype(np.float32)).to(dt), f, H, W))


def standin_input(name, u8, mutant=None):
    """fp32, tap by tap on the zero-extended staging row (what frame_resample does).  Mutants: 'origin_sign' (origin subtracted),
    'hi_max' (high tap clamped to Hmax - 1 / Wmax - 1, not to the frame), 'edge_clamp' (edge pixel where zero belongs outside the
    buffer), 'halfpix' (half-pixel centres), 'align' (scale (h - 1) / (H - 1))."""
    Hm, Wm = INPUT_STAGING

    def one(row, frame, H, W):
        h, w, oy, ox = frame[:4]
        row = torch.from_numpy(row.astype(np.float32))
        if h == 0 or w == 0:
            return torch.zeros(H, W, 3)
        if mutant == 'origin_sign':
            oy, ox = -oy, -ox

        def axis(i, o, lim):
            s = (i - 1) / max(o - 1, 1) if mutant == 'align' else i / o
            src = torch.arange(o, dtype=F32) * s
            if mutant == 'halfpix':
                src = ((torch.arange(o, dtype=F32) + 0.5) * s - 0.5).clamp(min=0.0)
            lo = torch.floor(src)
            return lo.long(), torch.clamp(lo + 1, max=(lim if mutant == 'hi_max' else i) - 1).long(), src - lo

        ylo, yhi, yl = axis(h, H, Hm - oy)
        xlo, xhi, xl = axis(w, W, Wm - ox)

        def tap(yy, xx):
            r, c = (yy + oy).view(-1, 1), (xx + ox).view(1, -1)
            v = row[r.clamp(0, Hm - 1), c.clamp(0, Wm - 1)]
            if mutant == 'edge_clamp':
                return v
            return v * ((r >= 0) & (r < Hm) & (c >= 0) & (c < Wm)).unsqueeze(2)

        xl_ = xl.view(1, -1, 1)
        t = tap(ylo, xlo) + (tap(ylo, xhi) - tap(ylo, xlo)) * xl_
        b = tap(yhi, xlo) + (tap(yhi, xhi) - tap(yhi, xlo)) * xl_
        return (t + (b - t) * yl.view(-1, 1, 1)) / 255.0 - _mean(F32)

    return _input_rows(name, u8, one)


def check_input(got3, name, u8):
    """got3 [2B, H, W, 3].  Empty slots exactly 0; the rest inside max(1e-6, 2 x fp32 oracle).  Returns (worst, oracle's, bound)."""
    got3 = got3.detach().cpu()
    frames, _ = INPUT_CASES[name]
    B = len(frames)
    r32, r64 = ref_input(name, u8, F32), ref_input(name, u8, F64)
    for b, f in enumerate(frames):
        if f[0] == 0:
            assert bool((got3[b] == 0).all()) and bool((got3[B + b] == 0).all()), "an empty slot's rows are exactly 0"
    bound, own = L.grad_bound(r32, r64, floor=FLOOR)
    return L.check_grad(got3, r64, bound), own, bound


# ================================================================================================ 4. unflow_inference_output
OUT_NET = (32, 64)
# (h, w, y0, x0, nmaps); (29, 37) at (-3, 60): part of its ground truth lies outside the buffer; (37, 83): larger than the network
OUT_FRAMES_88 = [(19, 45, 2, 3, 2), (29, 37, -3, 60, 2), (32, 64, 0, 0, 1), (1, 1, 5, 5, 2), (1, 45, 39, 40, 0), (37, 83, 3, 5, 2),
                 (0, 0, 0, 0, 2)]
# the frames of the list that fit a 24 x 40 row are (1, 1) and the empty slot alone: (19, 33) and the whole row added
OUT_FRAMES_40 = [(1, 1, 5, 5, 2), (19, 33, -2, 3, 2), (24, 40, 0, 0, 1), (0, 0, 0, 0, 2)]
# name -> (staging, flow size, frames, flow_scale, with metrics)
OUT_CASES = {
    'nb1_flow2': ((24, 40), (8, 16), OUT_FRAMES_40, 20.0, True),
    'nb1_flow0': ((24, 40), (32, 64), OUT_FRAMES_40, 20.0, True),
    'nb4_flow2': ((40, 88), (8, 16), OUT_FRAMES_88, 20.0, True),
    'nb4_flow0': ((40, 88), (32, 64), OUT_FRAMES_88, 20.0, True),
    # a flow that is no integer fraction of the network: only there does the two-stage resize differ from a single one
    'nb4_ragged': ((40, 88), (5, 12), OUT_FRAMES_88, 20.0, True),
    'saturate': ((40, 88), (8, 16), OUT_FRAMES_88, 2000.0, False),
    # 1,054,720 px: unflow_inference_output_blocks caps at 1024, the final reduction's j += 256 loop makes four rounds
    # (flow_scale 1: the frame is 16 x 32 times the network, the frame-size flow stays at tens of pixels)
    'cap': ((1030, 1024), (8, 16), [(1030, 1024, 0, 0, 2)], 1.0, True),
}
OUT_SUM_REL = 1e-5
OUT_THR_MARGIN = 1e-3
OUT_THR_SHARE_CAP = 2e-3
OUT_U16_SENTINEL = 0x1234


def out_blocks(Hm, Wm):
    """unflow_inference_output_blocks."""
    return max(1, min((Hm * Wm + 1023) // 1024, 1024))


def oracle_output(flow_b, h, w, scale):
    """flow_b [1, fh, fw, 2] -> the frame-size flow [h, w, 2]: final_flows()' resize * scale to the network size (flow * scale when
    it is there already), then resize_output_flow's resize to (h, w) and per-axis rescale."""
    H, W = OUT_NET
    dt = flow_b.dtype
    mid = flow_b * scale if tuple(flow_b.shape[1:3]) == (H, W) else M.resize_bilinear_tf1(flow_b, H, W) * scale
    return M.resize_bilinear_tf1(mid, h, w)[0] * torch.tensor([w / W, h / H], dtype=F64).to(dt)


@functools.lru_cache(maxsize=None)
def make_output_case(name):
    """flow [B, fh, fw, 2] (noise on a smooth field of up to 4 * flow_scale px: the 5 % term of the outlier threshold acts), and
    with metrics gt [2, B, Hmax, Wmax, 2] = the fp64 frame flow + 3 px noise placed at each frame's origin, mask [2, B, Hmax, Wmax]."""
    (Hm, Wm), (fh, fw), frames, scale, metrics = OUT_CASES[name]
    B = len(frames)
    g = torch.Generator().manual_seed(40 + fh + Hm)
    yy, xx = torch.meshgrid(torch.arange(fh, dtype=F32), torch.arange(fw, dtype=F32), indexing='ij')
    base = torch.stack([4.0 * torch.sin(xx * (6.0 / fw)), 2.0 * torch.cos(yy * (5.0 / fh))], 2)
    flow = base.unsqueeze(0) + torch.randn(B, fh, fw, 2, generator=g) * 0.4
    gt, mask = torch.zeros(2, B, Hm, Wm, 2), torch.zeros(2, B, Hm, Wm)
    if metrics:
        for b, (h, w, y0, x0, _) in enumerate(frames):
            if h == 0:
                continue
            f64 = oracle_output(flow[b:b + 1].double(), h, w, scale)
            for k in range(2):
                place_region(gt[k, b], (f64 + torch.randn(h, w, 2, generator=g, dtype=F64) * 3.0).float(), y0, x0)
                place_region(mask[k, b], (torch.rand(h, w, generator=g) < 0.6 - 0.1 * k).float(), y0, x0)
    return dict(flow=flow, gt=gt, mask=mask, desc=desc_rows(frames))


@functools.lru_cache(maxsize=None)
def ref_output(name, dt):
    """Per sample the [h, w, 2] flow (None for an empty slot)."""
    _, _, frames, scale, _ = OUT_CASES[name]
    flow = make_output_case(name)['flow'].to(dt)
    return [None if f[0] == 0 else oracle_output(flow[b:b + 1], f[0], f[1], scale) for b, f in enumerate(frames)]


def encode_u16(flow, dt=np.float32, rounding=False):
    """eval_gui.py flow_to_int16, restated: cast(max(0, min(x * 64 + 32768, 65535))), truncating."""
    x = flow.astype(dt) * dt(64.0) + dt(32768.0)
    x = np.maximum(dt(0.0), np.minimum(x, dt(65535.0)))
    return (np.rint(x) if rounding else np.trunc(x)).astype(np.uint16)


def frame_gt(name, b, k, ignore_origin=False):
    """Ground truth k of sample b as the frame's pixels see it: ([h, w, 2], [h, w]) fp64 numpy, zero outside the buffer."""
    h, w, y0, x0, _ = OUT_CASES[name][2][b]
    c = make_output_case(name)
    if ignore_origin:
        y0 = x0 = 0
    return (frame_region(c['gt'][k, b], h, w, y0, x0).double().numpy(), frame_region(c['mask'][k, b], h, w, y0, x0).double().numpy())


def flow_metrics(flow, gt, mask, five_percent=True):
    """flow_util.py's error of one frame in the precision of `flow`: (d [h, w], thr [h, w])."""
    d = np.sqrt(((gt.astype(flow.dtype) - flow) ** 2).sum(-1)) * mask.astype(flow.dtype)
    thr = np.maximum(np.sqrt((gt.astype(flow.dtype) ** 2).sum(-1)) * flow.dtype.type(0.05), flow.dtype.type(3.0))
    return d, (thr if five_percent else np.full_like(thr, 3.0))


def standin_output(name, b, mutant=None):
    """What the kernel leaves for sample b, from the fp32 oracle: dict flow [h, w, 2] fp32 tensor, u16 [h, w, 3] uint16, and per
    ground-truth map k < nmaps (esum, msum, count).  Mutants: 'swap_r' (the per-axis factors swapped), 'one_stage' (one resize
    from the flow to (h, w)), 'round' (encoding rounds), 'thr3' (threshold 3.0 without the 5 % term), 'gt_origin' (ground truth
    read without the origin offset)."""
    (_, _), _, frames, scale, metrics = OUT_CASES[name]
    h, w, _, _, nmaps = frames[b]
    H, W = OUT_NET
    fb = make_output_case(name)['flow'][b:b + 1]
    if mutant == 'one_stage':
        flow = M.resize_bilinear_tf1(fb, h, w)[0] * scale * torch.tensor([w / W, h / H])
    elif mutant == 'swap_r':
        flow = oracle_output(fb, h, w, scale) / torch.tensor([w / W, h / H]) * torch.tensor([h / H, w / W])
    else:
        flow = oracle_output(fb, h, w, scale)
    f = flow.numpy()
    out = dict(flow=flow, u16=np.concatenate([encode_u16(f, rounding=mutant == 'round'), np.ones((h, w, 1), np.uint16)], 2), maps=[])
    for k in range(nmaps if metrics else 0):
        gt, mask = frame_gt(name, b, k, ignore_origin=mutant == 'gt_origin')
        d, thr = flow_metrics(f, gt.astype(np.float32), mask.astype(np.float32), five_percent=mutant != 'thr3')
        out['maps'].append((float(d.astype(np.float64).sum()), float(mask.sum()), int((d >= thr).sum())))
    return out


def check_output_frame(got, name, b):
    """Everything asserted of one sample: the flow per pixel inside max(1e-6, 2 x fp32 oracle) of the frame's max; the encoding
    equal to the truncating encoding of got's own flow and within 1 of the fp64 flow's; per map the error sum at rel 1e-5, the
    mask sum exact, the outlier count within the number of pixels whose fp64 error is within 1e-3 of the threshold (share capped).
    Returns dict(worst, own, bound, near_share, outlier_share)."""
    _, _, frames, _, metrics = OUT_CASES[name]
    h, w, _, _, nmaps = frames[b]
    r32, r64 = ref_output(name, F32)[b], ref_output(name, F64)[b]
    bound, own = L.grad_bound(r32, r64, floor=FLOOR)
    worst = L.check_grad(got['flow'], r64, bound)
    own_flow = got['flow'].detach().cpu().numpy()
    u16 = got['u16']
    assert u16.dtype == np.uint16 and np.array_equal(u16[..., :2], encode_u16(own_flow)), "the truncating encoding of the fp32 flow"
    assert (u16[..., 2] == 1).all()
    enc64 = encode_u16(r64.numpy(), np.float64).astype(np.int64)
    assert np.abs(u16[..., :2].astype(np.int64) - enc64).max() <= 1, "within 1 of the fp64 flow's encoding"
    res = dict(worst=worst, own=own, bound=bound, near=0.0, outliers=[], valid=[])
    assert len(got['maps']) == (nmaps if metrics else 0)
    for k, (esum, msum, count) in enumerate(got['maps']):
        gt, mask = frame_gt(name, b, k)
        d, thr = flow_metrics(r64.numpy(), gt, mask)
        L.check_loss(esum, d.sum(), OUT_SUM_REL) if d.sum() > 0 else None
        assert msum == mask.sum(), ("mask sum", msum, mask.sum())
        near = int((np.abs(d - thr) < OUT_THR_MARGIN).sum())
        assert near / d.size <= OUT_THR_SHARE_CAP, ("near-threshold share", near / d.size)
        assert abs(int(count) - int((d >= thr).sum())) <= near, ("outliers", count, int((d >= thr).sum()), near)
        res['near'] = max(res['near'], near / d.size)
        res['outliers'].append(int((d >= thr).sum()))
        res['valid'].append(int((mask > 0).sum()))
    return res


# ================================================================================================ 5. unflow_inference_occlusion
OCC_SENTINEL = 7
OCC_OUTSIDE = 1.0e6              # the flow rows outside a frame: a tap that reads there makes the pixel occluded
OCC_MARGIN = 1e-3
OCC_SHARE_CAP = 2e-3
# name -> (staging, frames (h, w, y0, x0, nmaps)).  'main': (19, 45) at (-2, 170): part of its ground truth outside the buffer; the
# last frame has one map only: not scored.  'tie': constant integer flows with |fw + bw|^2 = 2 = 0.01 * 150 + 0.5 exactly, in fp32
# and in fp64: '>' says visible on every pixel.
OCC_CASES = {
    'main': ((100, 208), [(19, 45, -2, 170, 2), (1, 37, 0, 0, 2), (23, 1, 0, 0, 2), (97, 203, 3, 5, 2), (100, 208, 0, 0, 2),
                          (0, 0, 0, 0, 2), (19, 45, 0, 0, 1)]),
    'tie': ((6, 8), [(5, 7, 0, 0, 2)]),
}


@functools.lru_cache(maxsize=None)
def make_occlusion_case(name):
    """fw, bw [B, Hmax, Wmax, 2] and gt_mask [2, B, Hmax, Wmax] (map 0: evaluated pixels, map 1: the non-occluded among them), at
    each frame's origin."""
    (Hm, Wm), frames = OCC_CASES[name]
    B = len(frames)
    g = torch.Generator().manual_seed(70 + Hm)
    fw, bw = torch.full((B, Hm, Wm, 2), OCC_OUTSIDE), torch.full((B, Hm, Wm, 2), OCC_OUTSIDE)
    gt = torch.zeros(2, B, Hm, Wm)
    for b, (h, w, y0, x0, _) in enumerate(frames):
        if h == 0:
            continue
        if name == 'tie':
            fw[b, :h, :w], bw[b, :h, :w] = torch.tensor([2.0, 8.0]), torch.tensor([-1.0, -9.0])
        else:
            yy, xx = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing='ij')
            base = torch.stack([4.0 * torch.sin(xx / 40.0) + 1.5, 2.0 * torch.cos(yy / 30.0) - 0.5], 2)
            f = base + 0.15 * torch.randn(h, w, 2, generator=g)
            r = -base + 0.15 * torch.randn(h, w, 2, generator=g)
            occ = torch.rand(h, w, generator=g) < 0.3
            f[occ] += 6.0 * torch.randn(int(occ.sum()), 2, generator=g)
            far = torch.rand(h, w, generator=g) < 0.02
            f[far] += 3000.0 * torch.randn(int(far.sum()), 2, generator=g)
            fw[b, :h, :w], bw[b, :h, :w] = f, r
        ev = (torch.rand(h, w, generator=g) < 0.6).float()
        place_region(gt[0, b], ev, y0, x0)
        place_region(gt[1, b], ev * (torch.rand(h, w, generator=g) < 0.7).float(), y0, x0)
    return dict(fw=fw, bw=bw, gt=gt, desc=desc_rows(frames))


def oracle_occlusion(fw, bw):
    """losses.py:125-134 on one frame's fields [1, h, w, 2]: (occ_fw, occ_bw, |lhs - rhs| of both) each [h, w]."""
    mag = 0.01 * (M.length_sq(fw) + M.length_sq(bw)) + 0.5
    lf, lb = M.length_sq(fw + M.image_warp(bw, fw)), M.length_sq(bw + M.image_warp(fw, bw))
    return (lf > mag)[0, ..., 0], (lb > mag)[0, ..., 0], torch.minimum((lf - mag).abs(), (lb - mag).abs())[0, ..., 0]


@functools.lru_cache(maxsize=None)
def ref_occlusion(name, dt):
    (_, _), frames = OCC_CASES[name]
    c = make_occlusion_case(name)
    return [None if f[0] == 0 else oracle_occlusion(c['fw'][b:b + 1, :f[0], :f[1]].to(dt), c['bw'][b:b + 1, :f[0], :f[1]].to(dt))
            for b, f in enumerate(frames)]


def occlusion_counts(occ_fw, name, b):
    """TP, FP, FN of a forward mask [h, w] bool (numpy) against sample b's ground-truth maps, as the kernel scores them."""
    h, w, y0, x0, _ = OCC_CASES[name][1][b]
    gt = make_occlusion_case(name)['gt']
    ev = frame_region(gt[0, b], h, w, y0, x0).numpy() == 1
    gocc = ev & (frame_region(gt[1, b], h, w, y0, x0).numpy() == 0)
    return [int((occ_fw & gocc).sum()), int((occ_fw & ev & ~gocc).sum()), int((~occ_fw & gocc).sum())]


def standin_occlusion(name, b, mutant=None):
    """(occ_fw, occ_bw) uint8 numpy [h, w] from the fp32 oracle's pieces.  Mutants: 'mag_warped' (the magnitude taken from the warped
    partner), 'ge' (>= where > belongs), 'clamp_max' (taps clamped to the staging row, not to the frame), 'same_field' (the warp
    samples the field it is displaced by)."""
    h, w = OCC_CASES[name][1][b][:2]
    c = make_occlusion_case(name)
    fw, bw = c['fw'][b:b + 1, :h, :w], c['bw'][b:b + 1, :h, :w]
    if mutant == 'clamp_max':
        wbw, wfw = M.image_warp(c['bw'][b:b + 1], c['fw'][b:b + 1])[:, :h, :w], M.image_warp(c['fw'][b:b + 1], c['bw'][b:b + 1])[:, :h, :w]
    elif mutant == 'same_field':
        wbw, wfw = M.image_warp(fw, fw), M.image_warp(bw, bw)
    else:
        wbw, wfw = M.image_warp(bw, fw), M.image_warp(fw, bw)
    mf = mb = 0.01 * (M.length_sq(fw) + M.length_sq(bw)) + 0.5
    if mutant == 'mag_warped':
        mf, mb = 0.01 * (M.length_sq(fw) + M.length_sq(wbw)) + 0.5, 0.01 * (M.length_sq(bw) + M.length_sq(wfw)) + 0.5
    lf, lb = M.length_sq(fw + wbw), M.length_sq(bw + wfw)
    cmp = torch.ge if mutant == 'ge' else torch.gt
    return cmp(lf, mf)[0, ..., 0].numpy().astype(np.uint8), cmp(lb, mb)[0, ..., 0].numpy().astype(np.uint8)


def check_occlusion_frame(occ_fw, occ_bw, counts, name, b):
    """Both masks bit for bit against fp64 outside the pixels where either inequality's two sides are within 1e-3 (share capped);
    counts (None: not scored) exact against occ_fw itself and within the near-pixel count of the reference mask's.  Returns
    (near share, occluded share of the fp64 forward mask)."""
    r_fw, r_bw, gap = ref_occlusion(name, F64)[b]
    near = (gap < OCC_MARGIN).numpy()
    if name == 'tie':                                       # constructed to be exact in every precision: nothing is excused
        assert bool((gap == 0).all())
        near = np.zeros_like(near)
    share = near.mean()
    assert share <= OCC_SHARE_CAP, ("near-threshold share", share)
    for got, ref, tag in ((occ_fw, r_fw, 'fw'), (occ_bw, r_bw, 'bw')):
        assert got.dtype == np.uint8 and got.shape == near.shape and set(np.unique(got)) <= {0, 1}, (tag, np.unique(got))
        n = int(((got != ref.numpy().astype(np.uint8)) & ~near).sum())
        assert n == 0, ("mask pixels differ", tag, n)
    if counts is not None:
        assert list(counts) == occlusion_counts(occ_fw.astype(bool), name, b), ("counts against the kernel's own mask", list(counts))
        for a, r in zip(counts, occlusion_counts(r_fw.numpy(), name, b)):
            assert abs(int(a) - r) <= int(near.sum()), ("counts against the reference mask", list(counts))
    return float(share), float(r_fw.float().mean())
