"""Oracle of the voxel patch augmentation (csrc/spatial.hip), written for this repository on scipy in fp64:
`scipy.ndimage.map_coordinates` (order 3 / 1 with mode='nearest' for the image; order 0, and batchgenerators' per-label order-1
loop, with mode='constant' for the labels) and `scipy.ndimage.gaussian_filter(mode='constant', truncate=4)` for the elastic field.
Next to it stands a numpy RESTATEMENT of the kernels' arithmetic (pad 12 + recursive prefilter + 64 separable taps, trilinear,
the taps of the Gaussian), run in fp64 to check the oracle's own claims and in fp32 as the yardstick: a kernel may miss the
fp64 oracle by at most 4 x what the fp32 restatement misses it by on the same input, floor 8 * 2^-24 = 4.8e-7 of the largest
magnitude (`bar`).  Measured pairs are printed and, when FSG_SPATIAL_PARITY names a file, appended to it."""
import functools
import os

import numpy as np
from scipy import ndimage as ndi

FLOOR = 8 * 2.0 ** -24
PAD = 12
POLE = np.sqrt(3.0) - 2.0
VOLUME = (2, 1, 20, 24, 70)      # W crosses a wave with a remainder, no axis is a multiple of 64, H != D
PATCH = (12, 14, 66)


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def volume(shape=VOLUME, seed=5):
    """unit-variance noise, lightly smoothed so that it has structure at the voxel scale; fp32 values held in fp64"""
    rng = np.random.RandomState(seed)
    v = ndi.gaussian_filter(rng.standard_normal(shape), (0, 0, .7, .7, .7))
    v = (v / v.std()).astype(np.float32).astype(np.float64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def labels(shape=VOLUME):
    """three slanted 2-voxel sheets (labels 1..3) and a blob (4), int64 (B, 1, D, H, W); item 1 is item 0 shifted"""
    B, _, D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros(shape, np.int64)
    for b in range(B):
        s = out[b, 0]
        s[np.abs(x - (.30 * W + .9 * y - .4 * z + 2 * b)) < 1.0] = 1
        s[np.abs(y - (.55 * H + .25 * x - .12 * W + .3 * z - b)) < 1.0] = 2
        s[np.abs(z - (.45 * D + .15 * x - .08 * W - .2 * y + b)) < 1.0] = 3
        s[(z - .7 * D) ** 2 + (y - .3 * H) ** 2 + ((x - .75 * W) / 2) ** 2 < 9 + 4 * b] = 4
    out.setflags(write=False)
    return out


def rotation(a0, a1, a2):
    """batchgenerators' rotation of ROW vectors by R0 @ R1 @ R2, as the matrix applied to a column vector"""
    c, s = np.cos, np.sin
    r0 = np.array([[1, 0, 0], [0, c(a0), -s(a0)], [0, s(a0), c(a0)]])
    r1 = np.array([[c(a1), 0, s(a1)], [0, 1, 0], [-s(a1), 0, c(a1)]])
    r2 = np.array([[c(a2), -s(a2), 0], [s(a2), c(a2), 0], [0, 0, 1]])
    return (r0 @ r1 @ r2).T


@functools.lru_cache(maxsize=None)
def parameter_set(k, shape=VOLUME, patch=PATCH):
    """set k = 0..3 -> dict of fp32 arrays for a batch of shape[0] items: matrix (B, 3, 3), centre (B, 3), elastic
    (B, 3, *patch), noise, sigma (B,), alpha (B,).  Angles up to 0.3, scale 0.8 .. 1.2, sigma 1.5 .. 3, displacements up to
    about 3 voxels; the centres sit a few voxels off the middle."""
    B = shape[0]
    rng = np.random.RandomState(100 + k)
    angles = [(.3, -.3, .3), (-.21, .3, .07), (.12, .05, -.3), (-.3, -.3, -.3)][k]
    scales = [(0.8, 1.2), (1.2, 0.93), (1.07, 0.8), (0.88, 1.13)][k]
    sigmas = [(1.5, 3.0), (2.2, 1.7), (3.0, 2.5), (1.9, 2.8)][k]
    matrix = np.stack([rotation(*(np.array(angles) * (1 if b % 2 == 0 else -.8))) * scales[b % 2] for b in range(B)])
    centre = np.stack([(np.array(shape[2:]) - 1) / 2 + rng.uniform(-2.5, 2.5, 3) for _ in range(B)])
    noise = rng.uniform(-1, 1, (B, 3) + tuple(patch)).astype(np.float32)
    sigma = np.array([sigmas[b % 2] for b in range(B)], np.float32)
    smooth = np.stack([gaussian(noise[b].astype(np.float64), float(sigma[b])) for b in range(B)])
    alpha = (rng.uniform(2.5, 3.2, B) / np.abs(smooth).reshape(B, -1).max(1)).astype(np.float32)
    elastic = (alpha.astype(np.float64)[:, None, None, None, None] * smooth).astype(np.float32)
    out = {"matrix": matrix.astype(np.float32), "centre": centre.astype(np.float32), "elastic": elastic, "noise": noise,
           "sigma": sigma, "alpha": alpha}
    for v in out.values():
        v.setflags(write=False)
    return out


def coordinates(matrix, centre, elastic, patch, dtype=np.float64):
    """(B, 3, *patch): matrix_b @ ((o - (patch - 1) / 2) + elastic_b(o)) + centre_b, summed in the kernel's order, in `dtype`"""
    B = matrix.shape[0]
    m, c = matrix.astype(dtype), centre.astype(dtype)
    grid = np.stack(np.meshgrid(*(np.arange(p, dtype=dtype) - dtype(.5) * dtype(p - 1) for p in patch), indexing="ij"))
    p = np.broadcast_to(grid, (B, 3) + tuple(patch)).astype(dtype)
    if elastic is not None:
        p = p + elastic.astype(dtype)
    out = np.empty_like(p)
    for b in range(B):
        for i in range(3):
            out[b, i] = ((m[b, i, 0] * p[b, 0] + m[b, i, 1] * p[b, 1]) + m[b, i, 2] * p[b, 2]) + c[b, i]
    return out


# ------------------------------------------------------------------------------------------------ the oracle (scipy, fp64)
def gaussian(x, sigma):
    """x (3, pd, ph, pw) or any array whose last three axes are spatial -> gaussian_filter over those axes, fp64"""
    return ndi.gaussian_filter(np.asarray(x, np.float64), (0,) * (x.ndim - 3) + (sigma,) * 3, mode="constant", cval=0, truncate=4)


def sample_image(vol, coords, order):
    """vol (B, C, D, H, W), coords (B, 3, ...) -> (B, C, ...) by map_coordinates(order, mode='nearest'), fp64"""
    return np.stack([np.stack([ndi.map_coordinates(vol[b, c].astype(np.float64), coords[b], order=order, mode="nearest")
                               for c in range(vol.shape[1])]) for b in range(vol.shape[0])])


def labels_order1(seg, coords):
    """batchgenerators' interpolate_img for a label map at order 1: for every label ascending, the voxels where the order-1
    interpolation of its indicator reaches 0.5 take the label (a later label overwrites an earlier one); seg (D, H, W)"""
    out = np.zeros(coords.shape[1:], np.int64)
    for c in np.unique(seg):
        w = ndi.map_coordinates((seg == c).astype(np.float64), coords, order=1, mode="constant", cval=0)
        out[w >= 0.5] = c
    return out


def label_weights(seg, coords):
    """(labels present, their order-1 weights (L, ...)) -- for the excuses"""
    ls = np.unique(seg)
    return ls, np.stack([ndi.map_coordinates((seg == c).astype(np.float64), coords, order=1, mode="constant", cval=0) for c in ls])


def sample_labels(seg, coords, order):
    """seg (B, Cs, D, H, W) integer, coords (B, 3, ...) -> (B, Cs, ...) int64, mode='constant', cval=0"""
    one = (lambda s, c: ndi.map_coordinates(s, c, order=0, mode="constant", cval=0).astype(np.int64)) if order == 0 else labels_order1
    return np.stack([np.stack([one(seg[b, c], coords[b]) for c in range(seg.shape[1])]) for b in range(seg.shape[0])])


def excused(seg, coords, order, eps=1e-3, eps_w=2e-3):
    """(B, ...) bool: voxels where fp32 coordinates may legitimately decide otherwise -- a coordinate within eps of 0 or n - 1
    (both orders), of a half-integer (order 0), or a label weight within eps_w of 0.5 (order 1)"""
    B = coords.shape[0]
    n = np.array(seg.shape[2:], np.float64).reshape(1, 3, *([1] * (coords.ndim - 2)))
    ex = ((np.abs(coords) < eps) | (np.abs(coords - (n - 1)) < eps)).any(1)
    if order == 0:
        ex |= (np.abs(coords - np.floor(coords) - 0.5) < eps).any(1)
    else:
        for b in range(B):
            for c in range(seg.shape[1]):
                ex[b] |= (np.abs(label_weights(seg[b, c], coords[b])[1] - 0.5) < eps_w).any(0)
    return ex


def resample_coords(size, spacing, target):
    """(output size, per-axis fp64 coordinates i * target / spacing) of resample_equal_spacing"""
    out = [round(s * sp / target) for s, sp in zip(size, spacing)]
    return out, [np.arange(o, dtype=np.float64) * (target / sp) for o, sp in zip(out, spacing)]


def resample(vol, spacing, target, nearest):
    """(D, H, W) -> the volume on the grid of resample_coords, edge-replicated, fp64"""
    size, axes = resample_coords(vol.shape, spacing, target)
    coords = np.stack(np.meshgrid(*axes, indexing="ij"))
    return ndi.map_coordinates(vol.astype(np.float64), coords, order=0 if nearest else 1, mode="nearest")


# ------------------------------------------------------------------------------------------------ the restatement (numpy)
def prefilter(vol, pad=PAD, dtype=np.float64):
    """vol (..., D, H, W) -> coefficients (..., D + 2 pad, H + 2 pad, W + 2 pad) in `dtype`: edge-pad, then per axis the
    recursion of scipy's spline_filter1d(order=3, mode='nearest') -- gain 6, whole-sample-symmetric causal start over the
    WHOLE line, anticausal start c[last] *= z / (z - 1)"""
    z = dtype(POLE)
    c = np.pad(vol.astype(dtype), [(0, 0)] * (vol.ndim - 3) + [(pad, pad)] * 3, mode="edge")
    for ax in (-1, -2, -3):
        c = np.moveaxis(c, ax, 0).copy()
        n = c.shape[0]
        c *= dtype(6)
        zn = z ** n
        zi = z
        first = c[0].copy()
        acc = c[0] + zn * c[n - 1]
        for i in range(1, n):
            acc = acc + zi * (c[i] + zn * c[n - 1 - i])
            zi = zi * z
        c[0] = acc * (z / (dtype(1) - zn * zn)) + first
        for i in range(1, n):
            c[i] = c[i] + z * c[i - 1]
        c[n - 1] = c[n - 1] * (z / (z - dtype(1)))
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
        c = np.moveaxis(c, 0, ax)
    return np.ascontiguousarray(c)


def cubic_weights(t):
    u = 1 - t
    six, two, three, four = (t.dtype.type(v) for v in (6, 2, 3, 4))
    return [u * u * u / six, (t * t * (t - two) * three + four) / six, (u * u * (u - two) * three + four) / six, t * t * t / six]


def cubic(coef, coords, pad=PAD):
    """coef (Dp, Hp, Wp), coords (3, ...) in image units, both of one dtype -> 64 separable taps at coordinate + pad, tap indices
    clamped to the padded array (scipy's rule: beyond the padding the value runs into the edge coefficient)"""
    dt = coef.dtype.type
    w, idx = [], []
    for ax in range(3):
        n = coef.shape[ax]
        q = np.clip(coords[ax] + dt(pad), dt(-2), dt(n + 1))
        g = np.floor(q)
        w.append(cubic_weights(q - g))
        idx.append([np.clip(g.astype(np.int64) - 1 + j, 0, n - 1) for j in range(4)])
    out = np.zeros(coords.shape[1:], coef.dtype)
    for jz in range(4):
        az = np.zeros_like(out)
        for jy in range(4):
            ax_ = np.zeros_like(out)
            for jx in range(4):
                ax_ = ax_ + w[2][jx] * coef[idx[0][jz], idx[1][jy], idx[2][jx]]
            az = az + w[1][jy] * ax_
        out = out + w[0][jz] * az
    return out


def trilinear(vol, coords):
    """vol (D, H, W), coords (3, ...) of one dtype -> trilinear on the coordinate clamped to [0, n - 1]"""
    dt = vol.dtype.type
    i0, i1, t = [], [], []
    for ax in range(3):
        n = vol.shape[ax]
        q = np.clip(coords[ax], dt(0), dt(n - 1))
        g = np.floor(q)
        t.append(q - g)
        i0.append(g.astype(np.int64))
        i1.append(np.minimum(g.astype(np.int64) + 1, n - 1))
    one = dt(1)

    def lerp(a, b, f):
        return a * (one - f) + b * f
    x = [[lerp(vol[z, y, i0[2]], vol[z, y, i1[2]], t[2]) for y in (i0[1], i1[1])] for z in (i0[0], i1[0])]
    return lerp(lerp(x[0][0], x[0][1], t[1]), lerp(x[1][0], x[1][1], t[1]), t[0])


def restate_image(vol, matrix, centre, elastic, patch, order, dtype):
    """the whole image path in `dtype`: (B, C, *patch)"""
    coords = coordinates(matrix, centre, elastic, patch, dtype)
    src = prefilter(vol, dtype=dtype) if order == 3 else vol.astype(dtype)
    f = cubic if order == 3 else trilinear
    return np.stack([np.stack([f(src[b, c], coords[b]) for c in range(vol.shape[1])]) for b in range(vol.shape[0])])


def gauss_taps(sigma, dtype):
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1).astype(dtype)
    w = np.exp(dtype(-0.5) / (dtype(sigma) * dtype(sigma)) * (x * x))
    return (w / w.sum(dtype=dtype)).astype(dtype), r


def restate_gaussian(x, sigma, alpha, dtype):
    """alpha * the three zero-padded tap passes (W, H, D) over the last three axes of x, in `dtype`"""
    w, r = gauss_taps(dtype(sigma), dtype)
    y = x.astype(dtype)
    for ax in (-1, -2, -3):
        y = np.moveaxis(y, ax, -1)
        n = y.shape[-1]
        p = np.concatenate([np.zeros(y.shape[:-1] + (r,), dtype), y, np.zeros(y.shape[:-1] + (r,), dtype)], -1)
        acc = np.zeros_like(y)
        for k in range(2 * r + 1):
            acc = acc + w[k] * p[..., k:k + n]
        y = np.moveaxis(acc, -1, ax)
    return dtype(alpha) * y


# ------------------------------------------------------------------------------------------------ the bar
def record(line):
    print(line)
    path = os.environ.get("FSG_SPATIAL_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def bar(label, got, want64, want32):
    """|got - oracle64| <= max(4 |restatement32 - oracle64|, FLOOR * magnitude), maxima over all entries, the magnitude the
    largest |oracle64| -> (ok, message); records the measured pair"""
    got, want64, want32 = (np.asarray(v, np.float64) for v in (got, want64, want32))
    mag = float(np.abs(want64).max())
    err, own = float(np.abs(got - want64).max()), float(np.abs(want32 - want64).max())
    rel = (lambda v: v / mag) if mag > 0 else (lambda v: v)
    record(f"SPATIAL_PARITY {label}: err {rel(err):.3e} restatement32 {rel(own):.3e} magnitude {mag:.3e}")
    return err <= max(4 * own, FLOOR * mag), f"{label}: err {err:.3e}, restatement32 {own:.3e}, magnitude {mag:.3e}"
