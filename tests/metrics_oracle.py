"""CPU oracle of fissure_segmentation_amd.metrics, written from the geometry (open3d is not available, so the reference's own
point_surface_distance cannot run; what pins this file is the closed-form cases of tests/test_metrics_cpu.py).

* `tri_dist2`: squared distance from points to triangles in fp64, straight from the definition -- the foot of the
  perpendicular if it falls inside the triangle (barycentric coordinates from the 2 x 2 Gram system), else the nearest of the
  three edge segments, each measured from its own end points.  A triangle without area has no interior and is its edges.
* `point_mesh_dist2`: its minimum over all faces of a mesh (lowest face index on ties), in chunks of queries.
* `kernel_order_dist2`: the same quantity in fp32 with the operation order of csrc/point_mesh.hip (the four-candidate form,
  every fma where the kernel has one), to tell the kernel's rounding from an error.
* the summary functions of metrics.py:96-153 restated, and the seeded inputs the tests and tools/make_golden_metrics.py share.
"""
import numpy as np
import torch


def _dot(a, b):
    return (a * b).sum(-1)


def _segment_dist2(p, a, b):
    ab = b - a
    ll = _dot(ab, ab)
    t = torch.where(ll > 0, _dot(p - a, ab) / torch.where(ll > 0, ll, torch.ones_like(ll)), torch.zeros_like(ll)).clamp(0, 1)
    r = p - (a + t[..., None] * ab)
    return _dot(r, r)


def tri_dist2(p, a, b, c):
    """p, a, b, c (..., 3) broadcastable, any float dtype (meant for fp64) -> squared distance from p to triangle abc"""
    ab, ac, ap = b - a, c - a, p - a
    e00, e01, e11 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
    det = e00 * e11 - e01 * e01
    has_area = det > 1e-24 * e00 * e11
    safe = torch.where(has_area, det, torch.ones_like(det))
    d1, d2 = _dot(ap, ab), _dot(ap, ac)
    v, w = (e11 * d1 - e01 * d2) / safe, (e00 * d2 - e01 * d1) / safe
    foot = ap - v[..., None] * ab - w[..., None] * ac
    inside = has_area & (v >= 0) & (w >= 0) & (v + w <= 1)
    edges = torch.minimum(torch.minimum(_segment_dist2(p, a, b), _segment_dist2(p, a, c)), _segment_dist2(p, b, c))
    return torch.where(inside, _dot(foot, foot), edges)


def point_mesh_dist2(pts, verts, faces, dtype=torch.float64, chunk=None):
    """pts (P,3), verts (V,3), faces (F,3) -> (min squared distance (P,), face index (P,) int64, lowest on ties)"""
    pts, verts = torch.as_tensor(pts).to(dtype), torch.as_tensor(verts).to(dtype)
    tri = verts[torch.as_tensor(faces).long()]                           # (F,3,3)
    chunk = chunk or max(1, 2_000_000 // max(1, len(tri)))
    best, arg = [], []
    for i in range(0, len(pts), chunk):
        d = tri_dist2(pts[i:i + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        m = d.min(1).values
        best.append(m)
        arg.append((d == m[:, None]).to(torch.uint8).argmax(1))       # first face that attains the minimum
    return torch.cat(best), torch.cat(arg)


def point_face_dist2(pts, verts, faces, face_index, dtype=torch.float64):
    """squared distance from pts[i] to the single face face_index[i]"""
    pts, verts = torch.as_tensor(pts).to(dtype), torch.as_tensor(verts).to(dtype)
    tri = verts[torch.as_tensor(faces).long()[torch.as_tensor(face_index).long()]]
    return tri_dist2(pts, tri[:, 0], tri[:, 1], tri[:, 2])


def barycentric(x, verts, faces, face_index):
    """fp64 least-squares coordinates (s, t) of x - a in the basis (ab, ac) of its face, and the distance of x to that plane
    point: x = a + s ab + t ac + residual.  For faces with area."""
    x, verts = torch.as_tensor(x).double(), torch.as_tensor(verts).double()
    tri = verts[torch.as_tensor(faces).long()[torch.as_tensor(face_index).long()]]
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    st = torch.linalg.lstsq(torch.stack([ab, ac], -1), (x - a)[..., None]).solution[..., 0]
    res = (x - a) - st[:, :1] * ab - st[:, 1:] * ac
    return st[:, 0], st[:, 1], res.norm(dim=1)


# ---------------------------------------------------------------- fp32, in the kernel's operation order
def _f(x):
    return x.to(torch.float32)


def _fma(a, b, c):
    """fused multiply-add of fp32 operands: the product is exact in fp64, one rounding of the sum to fp64 before the one to fp32"""
    return _f(a.double() * b.double() + c.double())


def _dot3(a, b):
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def _cross(a, b):
    return torch.stack([_fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), _fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                        _fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1)


def kernel_order_dist2(pts, verts, faces, chunk=None):
    """fp32 restatement of point_mesh_kernel"""
    pts, verts = _f(torch.as_tensor(pts)), _f(torch.as_tensor(verts))
    tri = verts[torch.as_tensor(faces).long()]
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    bc = ac - ab
    e00, e01, e11, ebc = _dot3(ab, ab), _dot3(ab, ac), _dot3(ac, ac), _dot3(bc, bc)
    n = _cross(ab, ac)
    nn = _dot3(n, n)
    one, zero = torch.ones_like(nn), torch.zeros_like(nn)

    def recip(x, ok):
        return torch.where(ok, one / torch.where(ok, x, one), zero)
    inv = recip(nn, (nn > 1e-30) & (nn > _f(torch.tensor(1e-10)) * (e00 * e11)))

    def recip_up(x):
        r = recip(x, x > 1e-30)
        return torch.where((x > 1e-30) & (x * r < 1), torch.nextafter(r, torch.full_like(r, float("inf"))), r)
    i00, i11, ibc = recip_up(e00), recip_up(e11), recip_up(ebc)
    m1, m2, k = _cross(ac, n) * inv[:, None], _cross(n, ab) * inv[:, None], e00 - e01
    chunk = chunk or max(1, 1_000_000 // max(1, len(tri)))
    out = []
    for i in range(0, len(pts), chunk):
        p = pts[i:i + chunk, None, :] - a[None]

        def resid2(s, t):
            r = torch.stack([_fma(-t, ac[None, :, j].expand_as(t), _fma(-s, ab[None, :, j].expand_as(s), p[..., j])) for j in range(3)], -1)
            return _dot3(r, r)
        d1, d2 = _dot3(p, ab[None].expand_as(p)), _dot3(p, ac[None].expand_as(p))
        v = _dot3(p, m1[None].expand_as(p)).clamp(0, 1)
        w = torch.minimum(_dot3(p, m2[None].expand_as(p)).clamp(min=0), 1 - v)
        tab, tac, tbc = (d1 * i00).clamp(0, 1), (d2 * i11).clamp(0, 1), (((d2 - d1) + k) * ibc).clamp(0, 1)
        z = torch.zeros_like(tab)
        d = torch.minimum(torch.minimum(resid2(v, w), resid2(tab, z)), torch.minimum(resid2(z, tac), resid2(1 - tbc, tbc)))
        out.append(d.min(1).values)
    return torch.cat(out)


# ---------------------------------------------------------------- summaries (metrics.py:96-153)
def symmetric_point_distances(d1, d2):
    d1, d2 = torch.as_tensor(d1), torch.as_tensor(d2)
    n = lambda d: d.numpy().astype(np.float64)  # noqa: E731
    q = lambda d: float(torch.quantile(d, 0.95))  # noqa: E731  (linear interpolation between order statistics)
    return tuple(torch.tensor(x) for x in ((n(d1).mean() + n(d2).mean()) / 2, (n(d1).std(ddof=1) + n(d2).std(ddof=1)) / 2,
                                           (n(d1).max() + n(d2).max()) / 2, (q(d1) + q(d2)) / 2))


def assd(vx, fx, vy, fy, dtype=torch.float64):
    """(mean, std, hd, hd95) of one mesh pair from oracle distances"""
    dxy = point_mesh_dist2(vx, vy, fy, dtype)[0].sqrt()
    dyx = point_mesh_dist2(vy, vx, fx, dtype)[0].sqrt()
    return symmetric_point_distances(dxy, dyx)


def batch_dice(pred, targ, n_labels):
    pred, targ = np.asarray(pred).reshape(len(pred), -1), np.asarray(targ).reshape(len(targ), -1)
    out = np.zeros((len(pred), n_labels))
    for lab in range(n_labels):
        p, t = pred == lab, targ == lab
        out[:, lab] = 2.0 * (p & t).sum(1) / (p.sum(1) + t.sum(1) + 1e-8)
    return out.mean(0)


def binary_recall(pred, targ):
    p, t = np.asarray(pred).reshape(len(pred), -1) != 0, np.asarray(targ).reshape(len(targ), -1) != 0
    return ((p & t).sum(1) + 1e-8) / (t.sum(1) + 1e-8)


def binary_precision(pred, targ):
    p, t = np.asarray(pred).reshape(len(pred), -1) != 0, np.asarray(targ).reshape(len(targ), -1) != 0
    return ((p & t).sum(1) + 1e-8) / (p.sum(1) + 1e-8)


# ---------------------------------------------------------------- seeded inputs
def plane_faces(s):
    """the face list of shapes.shape_constructor.get_plane_mesh for an s x s vertex grid: two triangles per cell"""
    cell = (np.arange(s - 1)[:, None] * s + np.arange(s - 1)[None, :]).reshape(-1)
    return np.stack([np.stack([cell, cell + 1, cell + s], 1), np.stack([cell + 1, cell + s, cell + 1 + s], 1)], 1).reshape(-1, 3)


def height_field_mesh(seed, B, s):
    """(verts (B, s*s, 3) fp32, faces (2 (s-1)^2, 3) int64): the s x s grid over [-1, 1]^2 lifted to the noisy height field of
    oracle/make_golden_mesh.surface_samples, z = a sin(3x) cos(2y) + 0.01 N(0,1), one amplitude per mesh"""
    rng = np.random.default_rng(seed)
    g = np.linspace(-1, 1, s)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(1, -1, 2).repeat(B, 0)
    amp = rng.uniform(0.1, 0.4, (B, 1))
    z = amp * np.sin(3 * xy[..., 0]) * np.cos(2 * xy[..., 1]) + 0.01 * rng.standard_normal((B, s * s))
    return np.concatenate([xy, z[..., None]], -1).astype(np.float32), plane_faces(s)


def height_field_points(seed, B, n):
    """(B, n, 3) fp32 samples of the same kind of surface at uniform (x, y)"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (B, n, 2))
    amp = rng.uniform(0.1, 0.4, (B, 1))
    z = amp * np.sin(3 * xy[..., 0]) * np.cos(2 * xy[..., 1]) + 0.01 * rng.standard_normal((B, n))
    return np.concatenate([xy, z[..., None]], -1).astype(np.float32)


SUMMARY_SEED, SUMMARY_N1, SUMMARY_N2 = 1201, 1000, 777
LABEL_SEED, LABEL_B, LABEL_SHAPE, LABEL_N = 1202, 3, (6, 7, 5), 4


def summary_inputs():
    """two seeded fp32 distance sets (gamma-distributed, like surface distances: positive with a tail)"""
    rng = np.random.default_rng(SUMMARY_SEED)
    return rng.gamma(2.0, 0.01, SUMMARY_N1).astype(np.float32), rng.gamma(2.5, 0.012, SUMMARY_N2).astype(np.float32)


def label_inputs():
    """seeded (prediction, target) label maps (B, *shape) int64 with LABEL_N labels; the last item's target has no foreground"""
    rng = np.random.default_rng(LABEL_SEED)
    pred = rng.integers(0, LABEL_N, (LABEL_B,) + LABEL_SHAPE)
    targ = np.where(rng.random(pred.shape) < 0.7, pred, rng.integers(0, LABEL_N, pred.shape))
    targ[-1] = 0
    return pred.astype(np.int64), targ.astype(np.int64)
