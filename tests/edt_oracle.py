"""numpy / scipy restatement of the Euclidean distance transform of csrc/edt.hip, of `functional.nearest_label` and
`functional.labelmap_distances`, and of the lung split of data_processing/process_lung_mask.py, with the inputs their tests
share.  Test infrastructure, no test cases.
  edt_sq        scipy.ndimage.distance_transform_edt(mask, sampling) ** 2 in fp64: THE reference
  brute_sq      the definition, O(N^2), for tiny volumes: min over the zero voxels (sites) of the squared scaled offset
  passes        the kernel's three passes (W, H, D) with its arithmetic (int32 for unit spacing, else fp32 with separately
                rounded product, square and sum), its stop rule and its tie rule (smaller offset, then lower index), and the
                winning site's linear index
  lung_split    process_lung_mask.py:31-93 of the reference on scipy.ndimage with the package's ball (functional.ball_offsets)
"""
import numpy as np
from scipy import ndimage as ndi

INT_INF = np.int32(2 ** 31 - 1)


def edt_sq(mask, sampling=None):
    return ndi.distance_transform_edt(np.asarray(mask) != 0, sampling=sampling).astype(np.float64) ** 2


def brute_sq(mask, sampling=None):
    mask = np.asarray(mask) != 0
    s = np.ones(3) if sampling is None else np.asarray(sampling, np.float64)
    sites = np.argwhere(~mask).astype(np.float64)
    vox = np.argwhere(np.ones(mask.shape, bool)).astype(np.float64)
    if len(sites) == 0:
        return np.full(mask.shape, np.inf)
    d = ((vox[:, None, :] - sites[None, :, :]) * s) ** 2
    return d.sum(-1).min(1).reshape(mask.shape)


def _sq(delta, s, integer):
    if integer:
        return np.int32(delta * delta)
    d = np.float32(s) * np.float32(delta)
    return np.float32(d * d)


def _add(f, t, integer):
    if integer:
        return np.where(f == INT_INF, INT_INF, f.astype(np.int64) + np.int64(t)).astype(np.int32)
    with np.errstate(over="ignore"):
        return (f + t).astype(np.float32)


def _row_pass(mask, s, integer):
    """W pass: nearest site of the row; a tie goes to the left site -> (f, x of the site or -1)"""
    W = mask.shape[-1]
    x = np.broadcast_to(np.arange(W), mask.shape)
    site = ~mask
    left = np.maximum.accumulate(np.where(site, x, -1), axis=-1)
    right = np.minimum.accumulate(np.where(site, x, 2 * W)[..., ::-1], axis=-1)[..., ::-1]
    has_l, has_r = left >= 0, right < 2 * W
    take_l = has_l & (~has_r | (x - left <= right - x))
    q = np.where(take_l, left, np.where(has_r, right, -1))
    delta = np.abs(x - q)
    if integer:
        f = np.where(q >= 0, (delta * delta), INT_INF).astype(np.int32)
    else:
        d = (np.float32(s) * delta.astype(np.float32)).astype(np.float32)
        f = np.where(q >= 0, (d * d).astype(np.float32), np.float32(np.inf)).astype(np.float32)
    return f, q.astype(np.int64)


def _line_pass(f, axis, s, integer):
    """H or D pass along `axis`: every voxel walks outward, lower side first, strict improvement only, and stops at the first
    offset whose own term reaches its best -> (values, winning position along the axis)"""
    f = np.moveaxis(f, axis, 0)
    L = f.shape[0]
    best = f.copy()
    pos = np.broadcast_to(np.arange(L).reshape((L,) + (1,) * (f.ndim - 1)), f.shape)
    arg = pos.copy()
    live = np.ones(f.shape, bool)
    inf = INT_INF if integer else np.float32(np.inf)
    for d in range(1, L):
        t = _sq(d, s, integer)
        live &= t < best
        if not live.any():
            break
        for sign in (-1, 1):                                  # j - d before j + d; a position outside the line offers +inf
            cand = np.full_like(f, inf)
            if sign < 0:
                cand[d:] = _add(f[:-d], t, integer)
            else:
                cand[:-d] = _add(f[d:], t, integer)
            upd = live & (cand < best)
            best = np.where(upd, cand, best)
            arg = np.where(upd, pos + sign * d, arg)
    return np.moveaxis(best, 0, axis), np.moveaxis(arg, 0, axis)


def passes(mask, sampling=None):
    """mask (D, H, W), nonzero = set -> (d2 int32 or fp32, idx int64 linear index of the winning site, -1 where there is none)"""
    mask = np.asarray(mask) != 0
    D, H, W = mask.shape
    integer = sampling is None
    s = (1, 1, 1) if integer else tuple(np.float32(v) for v in sampling)
    f0, qx = _row_pass(mask, s[2], integer)
    f1, ay = _line_pass(f0, 1, s[1], integer)
    q1 = ay * W + np.take_along_axis(qx, ay, 1)
    f2, az = _line_pass(f1, 0, s[0], integer)
    q2 = az * (H * W) + np.take_along_axis(q1, az, 0)
    none = f2 == (INT_INF if integer else np.float32(np.inf))
    return f2, np.where(none, -1, q2)


def nearest_label(labels, candidates, sampling=None):
    """argmin over the candidates (ascending) of the reference transform of labels != c, as process_lung_mask.py:83-87; for
    unit spacing the squared distances are compared as integers"""
    cands = sorted(candidates)
    d = np.stack([edt_sq(labels != c, sampling) for c in cands])
    if sampling is None:
        d = np.rint(d).astype(np.int64)
    return np.asarray(cands)[np.argmin(d, 0)]


def quantile_linear(d, q):
    srt = np.sort(np.asarray(d, np.float64))
    pos = q * (len(srt) - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, len(srt) - 1)
    return srt[lo] + (srt[hi] - srt[lo]) * (pos - lo)


def labelmap_distances(a, b, spacing=(1., 1., 1.)):
    """metrics.py:79-101 of the reference with scipy's transform as the nearest-neighbour search -> (mean, std, hd, hd95) fp64"""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    if not a.any() or not b.any():
        return (np.nan,) * 4
    samp = tuple(spacing)[::-1]
    d_ab = ndi.distance_transform_edt(~b, sampling=samp)[a]
    d_ba = ndi.distance_transform_edt(~a, sampling=samp)[b]
    both = (d_ab, d_ba)
    return (sum(d.mean() for d in both) / 2, sum(d.std(ddof=1) for d in both) / 2, sum(d.max() for d in both) / 2,
            sum(quantile_linear(d, 0.95) for d in both) / 2)


# ------------------------------------------------------------------------------------------------------------ lung split
def ball(r):
    from fissure_segmentation_amd.functional import ball_offsets
    fp = np.zeros((2 * r + 1,) * 3, bool)
    o = ball_offsets(r).numpy() + r
    fp[o[:, 0], o[:, 1], o[:, 2]] = True
    return fp


def opening(a, r):
    return ndi.binary_dilation(ndi.binary_erosion(a, ball(r), border_value=0), ball(r), border_value=0)


def plausible(sizes, max_volume_ratio=10):
    """-> (plausible, warns)"""
    sizes = sorted(sizes, reverse=True)
    if len(sizes) < 2 or sizes[0] / sizes[1] > max_volume_ratio:
        return False, False
    return True, len(sizes) > 2


def maybe_detach(mask, radius=3, max_radius=8):
    """-> (labels, n, radii of the openings done, whether the warning was due); ValueError past the largest ball"""
    radii = []
    while True:
        lab, n = ndi.label(mask, ndi.generate_binary_structure(3, 1))
        ok, warn = plausible(np.bincount(lab.ravel(), minlength=n + 1)[1:].tolist())
        if ok:
            return lab, n, radii, warn
        if radius > max_radius:
            raise ValueError("could not be detached")
        mask = opening(mask, radius)
        radii.append(radius)
        radius += 2


def lung_split(mask, left_label=1, right_label=2):
    """-> (uint8 volume, radii of the openings done, warned)"""
    mask = np.asarray(mask) != 0
    lab, n, radii, warn = maybe_detach(mask)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    order = np.lexsort((np.arange(n), -sizes))[:2] + 1           # the two largest, ties by the smaller label
    two = np.zeros(lab.shape, np.int64)
    two[lab == order[0]], two[lab == order[1]] = 1, 2
    cx = [np.argwhere(two == l)[:, 2].mean() for l in (1, 2)]
    cur_right, cur_left = np.argsort(cx, kind="stable") + 1      # smaller x is right
    lr = np.zeros(lab.shape, np.int64)
    lr[two == cur_left], lr[two == cur_right] = 1, 2
    if radii:
        lr = nearest_label(lr, (1, 2))
        lr[~mask] = 0
    out = np.zeros(lab.shape, np.uint8)
    out[lr == 1], out[lr == 2] = left_label, right_label
    return out, radii, warn


# ---------------------------------------------------------------------------------------------------------- shared inputs
def random_sites(shape, density, seed):
    """mask (B, D, H, W) bool with about `density` of the voxels zero (sites), at least one per item"""
    rng = np.random.default_rng(seed)
    m = rng.random(shape) >= density
    for b in range(shape[0]):
        m[b][tuple(rng.integers(0, n) for n in shape[1:])] = False
    return m


def _ellipsoid(shape, centre, semi):
    g = np.mgrid[tuple(slice(0, n) for n in shape)].astype(np.float64)
    return sum(((g[i] - centre[i]) / semi[i]) ** 2 for i in range(3)) <= 1


LUNG_SHAPE = (24, 40, 64)


def lungs_bridged():
    """two ellipsoids (semi-axes >= 7) joined by a bar three voxels thick: one component; the radius-3 opening removes the bar"""
    m = _ellipsoid(LUNG_SHAPE, (12, 20, 16), (9, 14, 11)) | _ellipsoid(LUNG_SHAPE, (11, 19, 47), (8, 13, 10))
    m[11:14, 19:22, 16:48] = True
    return m


def lungs_speck():
    """two separate ellipsoids and a speck of 5 voxels: three components, plausible, with the warning"""
    m = _ellipsoid(LUNG_SHAPE, (12, 20, 16), (9, 14, 11)) | _ellipsoid(LUNG_SHAPE, (11, 19, 47), (8, 13, 10))
    m[2, 3, 30:35] = True
    return m


def one_ball():
    return _ellipsoid(LUNG_SHAPE, (12, 20, 32), (9, 9, 9))


LABEL_SHAPE = (20, 24, 66)


def label_scene(seed=5):
    """labels 1 and 2 in blobs with gaps (0) and a few voxels of a third label that is no candidate"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(LABEL_SHAPE, np.int32)
    lab[_ellipsoid(LABEL_SHAPE, (6, 8, 15), (4, 5, 9))] = 1
    lab[_ellipsoid(LABEL_SHAPE, (13, 15, 48), (5, 6, 12))] = 2
    lab[_ellipsoid(LABEL_SHAPE, (15, 5, 30), (2, 3, 4))] = 1
    lab[rng.random(LABEL_SHAPE) < 0.002] = 2
    lab[rng.random(LABEL_SHAPE) < 0.002] = 1
    lab[0, 0, 60:64] = 7
    return lab


def label_scene_symmetric():
    """label 1 up to x = 20, label 2 from x = 44: the whole plane x = 32 is 12 voxels from both and must get label 1"""
    lab = np.zeros(LABEL_SHAPE, np.int32)
    lab[:, :, :21] = 1
    lab[:, :, 44:] = 2
    return lab


def slabs(shape=(16, 20, 24)):
    a, b = np.zeros(shape, bool), np.zeros(shape, bool)
    a[3:6, 2:15, 4:20] = True
    b[8:10, 5:19, 1:17] = True
    b[4, 16:18, 20:23] = True
    return a, b
