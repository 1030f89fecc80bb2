"""scipy.ndimage restatement of the ball morphology, connected components and find_lobes of csrc/morphology.hip, and the
seeded inputs its tests share.  The semantics are the definition (SimpleITK is not part of the test environment; parity with
it is unpinned):
  ball(r)       offsets o with sum_i (o_i / (r_i + 0.5))^2 <= 1, r an int or (rz, ry, rx); an axis of radius 0 has o_i = 0 only
  dilate/erode  scipy's binary_dilation / binary_erosion with that footprint and border_value
  closing       zero-pad by r, dilate, erode, crop: the closing of the zero-extended infinite grid
  opening       dilate(erode(x, border 0), border 0)
  label         scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3) for connectivity 6 | 18 | 26
  find_lobes    data_processing/find_lobes.py:106-177 of the reference on numpy
"""
import numpy as np
from scipy import ndimage as ndi


def radius3(r):
    return (r, r, r) if isinstance(r, int) else tuple(r)


def ball(r):
    rz, ry, rx = radius3(r)
    g = np.mgrid[-rz:rz + 1, -ry:ry + 1, -rx:rx + 1].astype(np.float64)
    return (g[0] / (rz + 0.5)) ** 2 + (g[1] / (ry + 0.5)) ** 2 + (g[2] / (rx + 0.5)) ** 2 <= 1


def dilate(a, r, border=0):
    return ndi.binary_dilation(a, ball(r), border_value=border)


def erode(a, r, border=1):
    return ndi.binary_erosion(a, ball(r), border_value=border)


def closing(a, r):
    rz, ry, rx = radius3(r)
    p = np.pad(a, ((rz, rz), (ry, ry), (rx, rx)))
    c = erode(dilate(p, r, 0), r, 0)
    return c[rz:c.shape[0] - rz, ry:c.shape[1] - ry, rx:c.shape[2] - rx]


def opening(a, r):
    return dilate(erode(a, r, 0), r, 0)


def label(mask, connectivity=6):
    lab, n = ndi.label(mask, ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
    return lab.astype(np.int32), int(n)


def stats(lab, n):
    """-> sizes (n) int64, index sums (n, 3) int64 in (z, y, x) order, of the labels 1..n"""
    flat = lab.ravel()
    sizes = np.bincount(flat, minlength=n + 1)[1:n + 1].astype(np.int64)
    idx = np.indices(lab.shape).reshape(3, -1)
    sums = np.stack([np.bincount(flat, weights=idx[a].astype(np.float64), minlength=n + 1)[1:n + 1] for a in range(3)], 1)
    return sizes, np.rint(sums).astype(np.int64)   # (fp64 sums of integers below 2^53: exact)


def size_order(sizes):
    """old labels - 1 in the order of the new ones: by size descending, ties by the smaller label first"""
    return np.lexsort((np.arange(len(sizes)), -sizes))


def relabel_by_size(lab, n):
    sizes, _ = stats(lab, n)
    lut = np.zeros(n + 1, np.int32)
    lut[size_order(sizes) + 1] = np.arange(1, n + 1)
    return lut[lab]


def find_lobes(fissures, lung, exclude_rhf=False):
    """-> (image, success): the component image (int32) if there are too few components, else the lobes (int64)"""
    f = fissures.copy()
    if exclude_rhf:
        f[f == 3] = 0                                                      # :108-110
    not_lobes = ~erode(lung != 0, 2, 1) | (f != 0)                         # :114-119
    not_lobes = dilate(closing(not_lobes, 2), 2, 0)                        # :122-123
    lobes_mask = opening(~not_lobes, 4)                                    # :127-128
    lab, n = label(lobes_mask, 6)                                          # :130-132
    target = 4 if exclude_rhf else 5
    if n < target:
        return lab, False
    sizes, sums = stats(lab, n)
    order = size_order(sizes)[:target]                                     # :141-148
    cen = sums[order].astype(np.float64) / sizes[order, None].astype(np.float64)   # (z, y, x); the reference's are (x, y, z)
    by_x = np.argsort(cen[:, 2], kind="stable")
    num_right = 2 if exclude_rhf else 3
    right, left = by_x[:num_right], by_x[num_right:]
    new = np.zeros(target, np.int64)
    lz = np.argsort(cen[left, 0], kind="stable")
    new[left[lz[0]]], new[left[lz[1]]] = 3, 4                              # :166-168
    rz = np.argsort(cen[right, 0], kind="stable")
    new[right[rz[0]]], new[right[rz[-1]]] = 1, 2                           # :170-172
    if not exclude_rhf:
        new[right[rz[1]]] = 5                                              # :174
    lut = np.zeros(n + 1, np.int64)
    lut[order + 1] = new
    return lut[lab], True


def multiple_objects_morphology(labelmap, r, mode):
    """utils/image_ops.py:31-47 as a sequential loop over the labels present, ascending"""
    out = labelmap.astype(np.uint8).copy()
    for i in np.unique(labelmap):
        if i == 0:
            continue
        obj = out == i
        if mode == "dilate":
            out[dilate(obj, r, 0)] = i
        else:
            out[obj & ~erode(obj, r, 1)] = 0
    return out


# ------------------------------------------------------------------------------------------------------ shared inputs
def lung_volume(shape=(72, 56, 112)):
    """two ellipsoid lungs, one tilted fissure plane in the left lung (label 1), two in the right (2 oblique, 3 horizontal)
    -> (lung bool, fissures uint8).  find_lobes gives 5 components of sizes 6923, 18425, 19638, 18425, 4192 (in label order;
    a size tie), 4 with the horizontal fissure excluded: 6923, 18425, 30895, 18425."""
    D, H, W = shape
    z, y, x = np.mgrid[:D, :H, :W].astype(np.float64)
    lung = np.zeros(shape, bool)
    fis = np.zeros(shape, np.uint8)
    for cx, side in ((W * 0.26, "R"), (W * 0.74, "L")):
        e = ((z - D / 2) / (D / 2 - 3)) ** 2 + ((y - H / 2) / (H / 2 - 3)) ** 2 + ((x - cx) / (W * 0.24 - 3)) ** 2 <= 1
        lung |= e
        if side == "L":
            f = np.abs((z - D / 2) + 0.3 * (y - H / 2)) < 0.6
            fis[e & f] = 1
        else:
            f = np.abs((z - D * 0.36) + 0.25 * (y - H / 2)) < 0.6
            fis[e & f] = 2
            g = np.abs((z - D * 0.68) - 0.1 * (y - H / 2)) < 0.6
            fis[e & g & ~f] = 3
    return lung, fis


def lung_volume_six():
    """lung_volume with a second, horizontal plane of label 1 low in the left lung: 6 components of sizes 6923, 1545, 9434,
    19638, 18425, 4192 (5 with the horizontal fissure of the right lung excluded), so find_lobes has to drop the smallest"""
    lung, fis = lung_volume()
    D, H, W = lung.shape
    z, _, x = np.mgrid[:D, :H, :W].astype(np.float64)
    fis[lung & (x > W / 2) & (np.abs(z - D * 0.28) < 0.6)] = 1
    return lung, fis


def lobe_numbering_holds(lobes, exclude_rhf=False):
    """the reference's numbering, checked from the voxels of the result alone (not the way find_lobes above derives it): the
    right lobes (1, 2 and, of five, 5) lie at smaller x than the left ones (3, 4); by z the right ones run 1 < (5 <) 2 and
    the left ones 3 < 4"""
    present = [1, 2, 3, 4] if exclude_rhf else [1, 2, 3, 4, 5]
    if sorted(np.unique(lobes).tolist()) != [0] + present:
        return False
    pos = {l: np.argwhere(lobes == l).mean(0) for l in present}   # (z, y, x)
    right = [1, 2] if exclude_rhf else [1, 5, 2]
    sides = max(pos[l][2] for l in right) < min(pos[3][2], pos[4][2])
    zs = [pos[l][0] for l in right]
    return bool(sides and all(a < b for a, b in zip(zs, zs[1:])) and pos[3][0] < pos[4][0])


def random_mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def serpentine(shape=(9, 33, 130)):
    """a one-voxel-wide path through the whole volume: every second row of every second slab, rows joined at alternating ends,
    slabs joined alternately at the end and at the start of the slab's path"""
    D, H, W = shape
    m = np.zeros(shape, bool)
    rows = list(range(0, H, 2))
    slab = np.zeros((H, W), bool)
    for yi, y in enumerate(rows):
        slab[y, :] = True
        if yi + 1 < len(rows):
            slab[y + 1, W - 1 if yi % 2 == 0 else 0] = True
    end = (rows[-1], W - 1 if len(rows) % 2 == 1 else 0)
    for zi, z in enumerate(range(0, D, 2)):
        m[z] = slab
        if z + 2 < D:
            m[(z + 1,) + (end if zi % 2 == 0 else (0, 0))] = True
    return m


def checkerboard(shape=(8, 8, 64)):
    z, y, x = np.indices(shape)
    return (z + y + x) % 2 == 0


def three_label_map(shape=(14, 20, 70)):
    """three blobs two to three voxels apart, so that their radius-2 dilations collide, and a thin plate that erosion removes"""
    m = np.zeros(shape, np.uint8)
    m[3:9, 4:10, 5:30] = 1
    m[3:9, 12:17, 8:33] = 2
    m[5:12, 6:15, 33:66] = 3
    m[12, 2:18, 60:69] = 2
    return m
