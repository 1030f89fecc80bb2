"""Point-cloud normal estimation on the GPU (csrc/pcl_normals.hip) against tests/normals_oracle.py under the project's bar
(dpsr_oracle.bar: 4 x the fp32 restatement's own error, floor 8 * 2^-24 x magnitude; the magnitude is 1 for the unit vectors
and the largest eigenvalue for the curvatures).  The kernel is fed the oracle's neighbour lists, so only the new code is under
test; one test runs the whole path through knn_segment.  Measured figures are printed as NORMALS_PARITY lines and kept in
profiles/normals_parity.txt.

Conditions on the inputs (checked on the fp64 oracle alone, never on the kernel's output): an eigenvector is ill-defined when
eigenvalues are close, so points with gap = (l1 - l0) / l2 < 0.05 are left out of the vector comparison (their curvatures are
still compared); the sign is compared only where margin = |2 n_pos - (k - 1)| > 2, where one borderline projection cannot decide
the flip; elsewhere vectors are compared up to sign.  At most 5 % of a case's points may be left out by either condition."""
import numpy as np
import pytest
import torch

import dpsr_oracle as do
import normals_oracle as no

pytestmark = pytest.mark.gpu
T = torch.from_numpy
TABLE = no.TABLE
FLOOR = do.FLOOR


def _dev():
    return torch.device("cuda:0")


def _F():
    from fissure_segmentation_amd import functional
    return functional


def _run(xyz, offset, K, idx=None, disambiguate=True, validate=False):
    """-> curvatures (n, 3), frames (n, 3, 3) as numpy; idx: the oracle's lists (-1 in unread columns is legal with validate=False)"""
    x = T(np.ascontiguousarray(xyz)).to(_dev())
    off = T(np.asarray(offset, np.int32)).to(_dev())
    i = None if idx is None else T(np.ascontiguousarray(idx).astype(np.int32)).to(_dev())
    curv, frames = _F().pointcloud_frames_packed(x, off, K, disambiguate, idx=i, validate=validate)
    assert curv.dtype == torch.float32 and frames.dtype == torch.float32 and not curv.requires_grad and not frames.requires_grad
    assert curv.shape == (len(xyz), 3) and frames.shape == (len(xyz), 3, 3)
    return curv.cpu().numpy(), frames.cpu().numpy()


def _align(v, ref):
    """v with the sign that brings it next to ref, row by row"""
    s = np.sign((v.astype(np.float64) * ref).sum(1, keepdims=True))
    return v * np.where(s == 0, 1.0, s)


def _compare(label, curv, frames, o64, o32, signed=True, cap_sign=True):
    """curvatures everywhere, normals where the gap allows, signed where the margin allows (or nowhere, signed=False)"""
    lam = float(o64["curvatures"].max())
    ok, msg = do.bar("NORMALS_PARITY", f"{label} curvatures", T(curv), T(o64["curvatures"]), T(o32["curvatures"]), lam)
    assert ok, msg
    keep = o64["gap"] >= 0.05
    assert (~keep).mean() <= 0.05, f"{label}: {(~keep).mean():.3f} of the points have gap < 0.05"
    firm = keep & (o64["margin"] > 2) if signed else np.zeros_like(keep)
    if signed and cap_sign:
        assert (o64["margin"] <= 2).mean() <= 0.05, f"{label}: {(o64['margin'] <= 2).mean():.3f} of the points have margin <= 2"
    want64 = o64["normals"]
    got = np.where(firm[:, None], frames[:, :, 0], _align(frames[:, :, 0], want64))
    want32 = np.where(firm[:, None], o32["normals"], _align(o32["normals"], want64))
    print(f"NORMALS_PARITY {label}: {len(keep)} points, {int((~keep).sum())} left out (gap), {int(firm.sum())} compared with sign")
    ok, msg = do.bar("NORMALS_PARITY", f"{label} normals", T(got[keep]), T(want64[keep]), T(want32[keep]), 1.0)
    assert ok, msg


def _frames_ok(label, frames):
    """columns orthonormal within 8 * 2^-24 * 4, y = z x n within the floor"""
    F64 = frames.astype(np.float64)
    ortho = np.abs(np.einsum("nij,nik->njk", F64, F64) - np.eye(3)).max()
    cross = np.abs(np.cross(F64[:, :, 2], F64[:, :, 0]) - F64[:, :, 1]).max()
    print(f"NORMALS_PARITY {label}: orthonormality defect {ortho:.3e}, |z x n - y| {cross:.3e}")
    assert ortho <= 4 * FLOOR and cross <= FLOOR, (ortho, cross)


# ------------------------------------------------------------------ 1. the ellipsoid table
@pytest.mark.parametrize("case", range(len(TABLE)))
def test_ellipsoid_table(case):
    n, k, sigma = TABLE[case]
    signed, cap_sign = [(True, True), (True, True), (True, True), (True, False), (False, False)][case]
    xyz = no.ellipsoid(n, sigma)
    o64, o32 = no.frames(xyz, k), no.frames(xyz, k, dtype=np.float32)
    curv, frames = _run(xyz, [n], k, o64["idx"])
    _compare(f"ellipsoid n={n} k={k}", curv, frames, o64, o32, signed, cap_sign)
    _frames_ok(f"ellipsoid n={n} k={k} frames", frames)
    if case == 0:
        # z, the eigenvector of the largest eigenvalue, up to sign.  Its own bar: a perturbation dC of the covariance turns an
        # eigenvector by at most |dC| / (absolute gap); the fp32 covariance and solve are good to a few ulp of l2, taken as the
        # floor 8 * 2^-24 l2, so the error is at most floor / gap_z where gap_z = (l2 - l1) / l2 >= 0.05
        keep = o64["gap_z"] >= 0.05
        assert keep.mean() >= 0.95
        z64 = o64["frames"][:, :, 2]
        err = np.abs(_align(frames[:, :, 2], z64) - z64).max(1)
        print(f"NORMALS_PARITY ellipsoid n={n} k={k} z: worst err * gap_z / floor {float((err * o64['gap_z'])[keep].max() / FLOOR):.3f}")
        assert (err[keep] <= FLOOR / o64["gap_z"][keep]).all()


# ------------------------------------------------------------------ 2. ragged packed cloud, k_s per segment, padded columns
def test_ragged_cloud_and_unread_columns():
    xyz, offset = no.ragged()
    K = 30
    o64, o32 = no.frames_packed(xyz, offset, K), no.frames_packed(xyz, offset, K, dtype=np.float32)
    idx = o64["idx"].copy()
    pad = idx < 0
    assert pad.any() and not pad[offset[3]:].any()           # the short segments have padded columns, the long ones none
    idx[pad] = 0                                             # as knn_segment might pad: some valid index
    curv, frames = _run(xyz, offset, K, idx)
    _compare("ragged K=30", curv, frames, o64, o32, signed=True, cap_sign=False)
    _frames_ok("ragged K=30 frames", frames)
    poison = idx.copy()
    poison[pad] = len(xyz) - 1                               # a point of the last segment, far from the short ones
    curv_p, frames_p = _run(xyz, offset, K, poison)
    assert np.array_equal(curv_p.view(np.uint32), curv.view(np.uint32))
    assert np.array_equal(frames_p.view(np.uint32), frames.view(np.uint32))
    # a poison index that IS read changes the row: the check above is not vacuous
    live = idx.copy()
    live[0, 1] = len(xyz) - 1
    curv_l, _ = _run(xyz, offset, K, live)
    assert not np.array_equal(curv_l[0], curv[0]) and np.array_equal(curv_l[1:], curv[1:])


def test_whole_path_through_knn_segment():
    """no idx given: knn_segment's lists on tie-free random input equal the oracle's own kNN, so the results meet the same bar"""
    sizes = [200, 300]
    rng = np.random.default_rng(7)
    xyz = np.concatenate([no.ellipsoid(s, 0.005, 20 + i) + rng.normal(scale=1e-4, size=(s, 3)).astype(np.float32)
                          for i, s in enumerate(sizes)])
    offset = np.cumsum(sizes).astype(np.int32)
    K = 16
    o64, o32 = no.frames_packed(xyz, offset, K), no.frames_packed(xyz, offset, K, dtype=np.float32)
    curv, frames = _run(xyz, offset, K)
    _compare("knn_segment path K=16", curv, frames, o64, o32)
    x = T(xyz).to(_dev())
    off = T(offset).to(_dev())
    idx, _ = _F().knn_segment(K, x, x, off, off)
    assert np.array_equal(idx.cpu().numpy(), o64["idx"])
    given = _run(xyz, offset, K, idx.cpu().numpy(), validate=True)
    assert np.array_equal(given[0], curv) and np.array_equal(given[1], frames)


# ------------------------------------------------------------------ 3. noisy flat sheet
def test_noisy_sheet_up_to_sign():
    xyz = no.sheet()
    o64, o32 = no.frames(xyz, 16), no.frames(xyz, 16, dtype=np.float32)
    curv, frames = _run(xyz, [len(xyz)], 16, o64["idx"])
    _compare("sheet n=512 k=16", curv, frames, o64, o32, signed=False)
    assert (np.abs(frames[:, 2, 0]) > 0.9).mean() > 0.95     # the normals are near +-e_z


# ------------------------------------------------------------------ 4. degenerate inputs
def _finite_unit(curv, frames, lam):
    assert np.isfinite(curv).all() and np.isfinite(frames).all()
    assert np.abs(np.linalg.norm(frames.astype(np.float64), axis=1) - 1).max() <= 4 * FLOOR
    assert curv.min() >= -FLOOR * max(lam, 1e-30)


def test_degenerate_neighbourhoods():
    k = 9
    # all neighbours coincident
    xyz = np.tile(np.float32([[0.3, -0.2, 0.1]]), (20, 1))
    idx = no.knn(xyz, k)
    curv, frames = _run(xyz, [20], k, idx)
    _finite_unit(curv, frames, 0.0)
    assert np.abs(curv).max() == 0
    # collinear neighbours
    t = np.sort(np.random.default_rng(5).uniform(-0.5, 0.5, 40))
    xyz = (t[:, None] * np.float64([[0.6, -0.3, 0.7]]) + 0.1).astype(np.float32)
    o64 = no.frames(xyz, k)
    curv, frames = _run(xyz, [40], k, o64["idx"])
    lam = float(o64["curvatures"].max())
    _finite_unit(curv, frames, lam)
    assert np.abs(curv[:, :2]).max() <= 4 * FLOOR * lam      # two vanishing eigenvalues (the coordinates are rounded to fp32)
    # exactly planar grid points: the normal is +-e_z exactly (within the floor), l0 within the floor of 0
    xyz = no.planar_grid()
    o64, o32 = no.frames(xyz, k), no.frames(xyz, k, dtype=np.float32)
    curv, frames = _run(xyz, [len(xyz)], k, o64["idx"])
    lam = float(o64["curvatures"].max())
    _finite_unit(curv, frames, lam)
    n = frames[:, :, 0]
    assert np.abs(np.abs(n[:, 2]) - 1).max() <= FLOOR and np.abs(n[:, :2]).max() <= FLOOR
    assert np.abs(curv[:, 0]).max() <= FLOOR * lam
    ok, msg = do.bar("NORMALS_PARITY", "planar grid curvatures", T(curv), T(o64["curvatures"]), T(o32["curvatures"]), lam)
    assert ok, msg


# ------------------------------------------------------------------ 5. one NaN point
def test_one_nan_point_stays_local():
    xyz = no.ellipsoid(300, 0.005, seed=9)
    k = 12
    idx = no.knn(xyz, k)
    bad = xyz.copy()
    bad[17] = np.nan
    curv, frames = _run(bad, [300], k, idx)
    lists_it = (idx == 17).any(1)
    assert 1 < lists_it.sum() < 100
    clean_c, clean_f = _run(xyz, [300], k, idx)
    assert np.isfinite(curv[~lists_it]).all() and np.isfinite(frames[~lists_it]).all()
    assert np.array_equal(curv[~lists_it], clean_c[~lists_it]) and np.array_equal(frames[~lists_it], clean_f[~lists_it])


# ------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_raise_before_any_launch():
    F = _F()
    cloud = T(no.ellipsoid(40, 0.005)).to(_dev())
    off = torch.tensor([40], dtype=torch.int32, device=_dev())
    for K in (1, 65):
        with pytest.raises(ValueError, match="neighborhood_size"):
            F.pointcloud_frames_packed(cloud, off, K)
        with pytest.raises(ValueError, match="neighborhood_size"):
            F.estimate_pointcloud_normals(cloud[None], K)
    for K in (40, 41):                                        # K >= N in the dense form
        with pytest.raises(ValueError, match="smaller than"):
            F.estimate_pointcloud_normals(cloud[None], K)
        with pytest.raises(ValueError, match="smaller than"):
            F.estimate_pointcloud_local_coord_frames(cloud[None], K)
    with pytest.raises(RuntimeError, match="(?i)GPU only"):
        F.estimate_pointcloud_normals(cloud[None].cpu(), 8)
    two = torch.tensor([20, 40], dtype=torch.int32, device=_dev())
    idx = T(no.frames_packed(cloud.cpu().numpy(), [20, 40], 8)["idx"]).to(_dev())
    F.pointcloud_frames_packed(cloud, two, 8, idx=idx, validate=True)                     # the good lists pass
    out_of_range, other_segment = idx.clone(), idx.clone()
    out_of_range[5, 3] = 40
    other_segment[5, 3] = 25                                  # row 5 belongs to segment 0 = points 0..19
    for bad in (out_of_range, other_segment):
        with pytest.raises(ValueError, match="segment"):
            F.pointcloud_frames_packed(cloud, two, 8, idx=bad, validate=True)
    with pytest.raises(ValueError, match="offset"):
        F.pointcloud_frames_packed(cloud, torch.tensor([20, 39], dtype=torch.int32, device=_dev()), 8, idx=idx, validate=True)
    with pytest.raises(ValueError, match="shape"):
        F.pointcloud_frames_packed(cloud, two, 8, idx=idx[:, :7])


# ------------------------------------------------------------------ 7. determinism, dense = packed
def test_deterministic_and_dense_equals_packed():
    F = _F()
    B, N, K = 3, 130, 30
    pts = np.stack([no.ellipsoid(N, 0.005, seed=30 + b) for b in range(B)])
    x = T(pts).to(_dev())
    off = torch.arange(1, B + 1, dtype=torch.int32, device=_dev()) * N
    c1, f1 = F.pointcloud_frames_packed(x.view(-1, 3), off, K)
    c2, f2 = F.pointcloud_frames_packed(x.view(-1, 3), off, K)
    assert torch.equal(c1, c2) and torch.equal(f1, f2)
    cd, fd = F.estimate_pointcloud_local_coord_frames(x, K)
    nd = F.estimate_pointcloud_normals(x, K)
    assert cd.shape == (B, N, 3) and fd.shape == (B, N, 3, 3) and nd.shape == (B, N, 3)
    assert torch.equal(cd.view(-1, 3), c1) and torch.equal(fd.view(-1, 3, 3), f1) and torch.equal(nd, fd[..., 0])
    assert not nd.requires_grad
    xg = x.clone().requires_grad_(True)
    assert not F.estimate_pointcloud_normals(xg, K).requires_grad           # constants: no gradient reaches the points
    # every neighbourhood size takes its own kernel instance: 16 / 32 / 64 are the borders
    for k in (16, 17, 32, 33, 64):
        o64, o32 = no.frames(pts[0], k), no.frames(pts[0], k, dtype=np.float32)
        curv, frames = _run(pts[0], [N], k, o64["idx"])
        _compare(f"ellipsoid n={N} k={k}", curv, frames, o64, o32, signed=True, cap_sign=False)


# ------------------------------------------------------------------ 8. without disambiguation
def test_without_disambiguation_up_to_sign():
    n, k, sigma = TABLE[1]
    xyz = no.ellipsoid(n, sigma)
    o64 = no.frames(xyz, k, disambiguate=False)
    o32 = no.frames(xyz, k, dtype=np.float32, disambiguate=False)
    curv, frames = _run(xyz, [n], k, o64["idx"], disambiguate=False)
    _compare(f"ellipsoid n={n} k={k} raw", curv, frames, o64, o32, signed=False)
    _frames_ok(f"ellipsoid n={n} k={k} raw frames", frames)
    flipped = _run(xyz, [n], k, o64["idx"], disambiguate=True)[1]
    same = np.abs(_align(flipped[:, :, 0], frames[:, :, 0].astype(np.float64)) - frames[:, :, 0]).max()
    assert same == 0                                          # the rule only ever changes a sign
