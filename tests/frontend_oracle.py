"""Oracle of the image front end: a restatement in torch on the CPU of the reference's Foerstner keypoints
(data_processing/foerstner.py), MIND descriptors (data_processing/point_features.py:86-150) and their helpers
(utils/image_utils.py, utils/general_utils.py), runnable in fp32 and fp64, plus the seeded inputs every test and
tools/make_golden_frontend.py share.  Constants that the reference fixes in fp32 (the Gaussian taps, the gradient stencil)
are computed in fp32 and then cast, so an fp64 run differs from an fp32 run by the rounding of the arithmetic alone.

tests/golden/frontend_*.npz hold what the REAL reference returned for these inputs; tests/test_frontend_cpu.py holds this
file to them."""
import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_SHAPE = (24, 28, 32)
LARGE_SHAPE = (96, 112, 128)
GOLDEN_SEED, LARGE_SEED = 3111, 3102
DIST_SIGMAS = (0.5, 1.4)
KPT_CONFIGS = ((0.5, 5), (1.4, 9), (0.5, 4))                  # (sigma, d)
MIND_CONFIGS = ((True, 1), (True, 2), (False, 1), (False, 2))   # (ssc, dilation)
PATCH_SIZES = (5, 4)
MIND_GOLDEN_PLANES = (0, 1, 2, 5, 8, 11, 14, 17, 20, 21, 22, 23)   # z planes of the MIND goldens that are stored (fixture size)
E2E_SHAPE, E2E_SEED = (32, 40, 48), 3215   # reject-sampled like GOLDEN_SEED: keypoint margin >= 1e-3 at (0.5, 5) inside the eroded mask
SIX = ((0, 1, 1), (1, 1, 0), (1, 0, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1))
SSC_PERMUTATION = (6, 8, 1, 11, 2, 10, 0, 7, 9, 4, 5, 3)


# ------------------------------------------------------------------ seeded inputs
def _box_blur(a, times):
    for _ in range(times):
        for ax in range(3):
            a = (np.roll(a, 1, ax) + a + np.roll(a, -1, ax)) / 3.0
    return a


def ct_volume(seed, shape=GOLDEN_SHAPE, constant_block=False):
    """smoothed noise scaled to CT-like magnitudes (about -1000 .. 400) -> (1, 1, D, H, W) fp32.  `constant_block`: one corner
    block is constant (0, so that its gradient is exactly 0 in every precision and summation order), as the padding of a
    real CT is: the distinctiveness is NaN there."""
    rng = np.random.default_rng(seed)
    a = _box_blur(rng.standard_normal(shape), 2)
    a = a / a.std()
    img = (-400.0 + 350.0 * a).astype(np.float32)
    if constant_block:
        d, h, w = shape
        img[: d // 3, : h // 3, : w // 3] = 0.0
    return torch.from_numpy(img)[None, None]


def box_mask(shape=GOLDEN_SHAPE, seed=None):
    """a box that touches two faces of the volume, with single-voxel holes and a few single voxels set outside it ->
    (1, 1, D, H, W) bool"""
    d, h, w = shape
    m = np.zeros(shape, dtype=bool)
    m[0: d - 3, 2: h - 2, 3: w] = True
    rng = np.random.default_rng(977 if seed is None else seed)
    n = max(8, d * h * w // 400)
    for z, y, x in zip(rng.integers(0, d, n), rng.integers(0, h, n), rng.integers(0, w, n)):
        m[z, y, x] = not m[z, y, x]
    return torch.from_numpy(m)[None, None]


def patch_points(seed, n, shape=GOLDEN_SHAPE):
    """n voxel positions (x, y, z), some on the border -> (n, 3) fp32"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    p = np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, d, n)], 1)
    p[0] = (0, 0, 0)
    p[1] = (w - 1, h - 1, d - 1)
    return torch.from_numpy(p.astype(np.float32))


# ------------------------------------------------------------------ filters
def gaussian_taps(sigma):
    s = torch.tensor([float(sigma)])
    n = int(torch.ceil(s * 3.0 / 2.0).long().item()) * 2 + 1
    w = torch.exp(-torch.pow(torch.linspace(-(n // 2), n // 2, n), 2) / (2 * torch.pow(s, 2)))
    return w / w.sum()


def filter_1d(img, weight, dim):
    B, C, D, H, W = img.shape
    n = weight.shape[0]
    pad = [0] * 6
    pad[4 - 2 * dim] = pad[5 - 2 * dim] = n // 2
    view = [1] * 5
    view[dim + 2] = -1
    return F.conv3d(F.pad(img.reshape(B * C, 1, D, H, W), pad, mode="replicate"), weight.to(img).view(view)).view(B, C, D, H, W)


def smooth(img, sigma):
    w = gaussian_taps(sigma)
    for dim in range(3):
        img = filter_1d(img, w, dim)
    return img


def nms(data, kernel_size):
    pad1 = kernel_size // 2
    pad2 = kernel_size - pad1 - 1
    return F.max_pool3d(F.pad(data, (pad2, pad1) * 3, mode="replicate"), kernel_size, stride=1)


# ------------------------------------------------------------------ Foerstner
def distinctiveness(img, sigma):
    filt = torch.tensor([1.0 / 12.0, -8.0 / 12.0, 0.0, 8.0 / 12.0, -1.0 / 12.0])
    g = [filter_1d(img, filt, k) for k in range(3)]
    a, b, c, e, f, i = (smooth(g[p] * g[q], sigma)[:, 0] for p in range(3) for q in range(p, 3))
    A = e * i - f * f
    B = - b * i + c * f
    C = b * f - c * e
    E = a * i - c * c
    I = a * e - b * b   # noqa: E741
    det = (a * A + b * B + c * C).unsqueeze(1)
    inv = (1. / det) * torch.stack([A, E, I], dim=1)
    return 1. / inv.sum(dim=1, keepdim=True)


def erode_mask(mask):
    """the reference's structuring element has a zero at its centre: a voxel survives iff none of its six face neighbours
    inside the volume is outside the mask, whatever the voxel itself is"""
    m = mask.bool()
    out = torch.ones_like(m)
    for ax in (2, 3, 4):
        n = m.shape[ax]
        out.narrow(ax, 1, n - 1).logical_and_(m.narrow(ax, 0, n - 1))
        out.narrow(ax, 0, n - 1).logical_and_(m.narrow(ax, 1, n - 1))
    return out


def keypoint_flags(dist, mask, d, thresh):
    return erode_mask(mask) & (nms(dist, d) == dist) & (dist >= thresh)


def foerstner_kpts(img, mask, sigma=1.4, d=9, thresh=1e-8):
    return torch.nonzero(keypoint_flags(distinctiveness(img, sigma), mask, d, thresh))[:, 2:]


def decision_margins(dist, d, thresh):
    """per voxel, the relative distance of the keypoint decision from flipping: |D - max of the REST of its window| / that
    maximum and |D - thresh| / thresh, whichever is smaller; inf where D is NaN or its window holds a NaN (no rounding
    changes those).  dist (1, 1, D, H, W) -> (D, H, W)"""
    pad1 = d // 2
    pad2 = d - pad1 - 1
    v, top = dist[0, 0], nms(dist, d)[0, 0]
    has_nan = torch.isnan(top)
    cand = torch.nonzero(v == top)                       # window maxima: the rest of their window decides
    if len(cand):
        r = torch.arange(d) - pad2
        offs = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).view(-1, 3)
        idx = cand[:, None, :] + offs[None]
        for ax in range(3):
            idx[..., ax].clamp_(0, v.shape[ax] - 1)      # replicate padding
        rest = v[idx[..., 0], idx[..., 1], idx[..., 2]]
        itself = (idx == cand[:, None, :]).all(-1)       # the centre, and its replicas at the border of the volume
        rest = torch.where(itself, torch.full_like(rest, float("-inf")), rest).max(-1).values
        top = top.clone()
        top[cand[:, 0], cand[:, 1], cand[:, 2]] = rest
    m = torch.minimum((v - top).abs() / top.abs(), (v - thresh).abs() / abs(thresh))
    return torch.where(has_nan | torch.isnan(m), torch.full_like(m, float("inf")), m)


# ------------------------------------------------------------------ MIND
def ssc_pairs():
    """the 12 (first, second) voxel pairs of the self-similarity context, as indices in {0, 1, 2}^3, in the reference's
    order before its final permutation: pairs (i, j) of the six-neighbourhood with i > j at squared distance 2"""
    return [(SIX[i], SIX[j]) for i in range(6) for j in range(6)
            if i > j and sum((a - b) ** 2 for a, b in zip(SIX[i], SIX[j])) == 2]


def mind(img, dilation=1, sigma=0.8, ssc=True):
    dt = img.dtype
    if ssc:
        pairs = ssc_pairs()
        k1, k2 = torch.zeros(12, 1, 3, 3, 3, dtype=dt), torch.zeros(12, 1, 3, 3, 3, dtype=dt)
        for c, (p, q) in enumerate(pairs):
            k1[c, 0][p] = 1
            k2[c, 0][q] = 1
    else:   # as the reference builds them: the first kernel all ones, the second indexed (channel, z, y) with whole x rows
        k1, k2 = torch.ones(6, 1, 3, 3, 3, dtype=dt), torch.zeros(6, 3, 3, 3, dtype=dt)
        six = torch.tensor(SIX)
        k2[six[:, 0], six[:, 1], six[:, 2]] = 1
        k2 = k2.unsqueeze(1)
    k1, k2 = k1.to(img.device), k2.to(img.device)
    p = F.pad(img, (dilation,) * 6, mode="replicate")
    m = smooth((F.conv3d(p, k1, dilation=dilation) - F.conv3d(p, k2, dilation=dilation)) ** 2, sigma)
    m = m - torch.min(m, 1, keepdim=True)[0]
    var = torch.mean(m, 1, keepdim=True)
    var = torch.clamp(var, var.mean() * 0.001, var.mean() * 1000)
    m = torch.exp(-(m / var))
    if ssc:
        m = m[:, torch.tensor(SSC_PERMUTATION, device=img.device)]
    return m


# ------------------------------------------------------------------ coordinates and patches
def kpts_to_grid(kpts_world, shape):
    D, H, W = shape
    whd = torch.tensor([W, H, D])
    return ((kpts_world * (1 / (whd - 1))) * 2 - 1) * ((whd - 1) / whd)


def kpts_to_world(kpts_pt, shape):
    D, H, W = shape
    whd = torch.tensor([W, H, D])
    return ((kpts_pt / ((whd - 1) / whd) + 1) / 2) * (whd - 1)


def sample_patches_at_kpts(img, kpts_grid, patch_size):
    g = F.affine_grid(torch.eye(3, 4).unsqueeze(0), size=[1, 1] + [patch_size] * 3, align_corners=False)
    g = g * (patch_size / torch.tensor(img.shape[2:][::-1]))
    n = kpts_grid.shape[0]
    g = (g + kpts_grid.view(n, 1, 1, 1, 3)).flatten(start_dim=1, end_dim=-2).view(1, n, patch_size ** 3, 1, 3)
    out = F.grid_sample(img, g.to(img.dtype), mode="nearest" if patch_size % 2 else "bilinear", padding_mode="border",
                        align_corners=False)
    return out.view(1, n, patch_size, patch_size, patch_size)


# ------------------------------------------------------------------ error statistics
def rel_err(got, want, denom_floor=1e-300):
    """(maximum, 99.9th percentile) of |got - want| / max(|want|, denom_floor) over the finite entries of `want` (fp64); NaN
    positions must coincide -> (max, p999, nan_positions_equal).  `denom_floor`: for fields bounded by 1 whose small values
    underflow in fp32 (MIND), below which the error counts as absolute."""
    got, want = got.double().flatten(), want.double().flatten()
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(want)))
    ok = torch.isfinite(want) & torch.isfinite(got)
    e = ((got[ok] - want[ok]).abs() / want[ok].abs().clamp_min(denom_floor)).numpy()
    if e.size == 0:
        return 0.0, 0.0, same_nan
    return float(e.max()), float(np.quantile(e, 0.999)), same_nan
