"""CPU tests of the surface-fitting feature (csrc/mesh_cleanup.hip, functional.orient_normals_consistent / mesh_face_components /
mesh_component_stats / mesh_remove_vertices, utils.general_utils.mask_out_verts_from_mesh / remove_all_but_biggest_component,
data_processing.pointcloud_surface_fitting.pointcloud_surface_fitting / fit_label_surfaces): the oracle of tests/surface_fit_oracle.py
against scipy and against cases worked out by hand -- it is what the kernels are held to on the GPU --, the C ABI's declarations
and host-side argument checks, and the host-side contract (imports without a GPU, refuses CPU tensors)."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

import mc_oracle
import normals_oracle
import surface_fit_oracle as so
from conftest import ROOT

NEW_SYMBOLS = ("fsg_orient_normals_workspace_bytes", "fsg_orient_normals_f32", "fsg_face_union_i32", "fsg_cluster_stats_f64",
               "fsg_mesh_keep_flags_u8", "fsg_mesh_face_flags_u8", "fsg_mesh_compact_f32")
P = 16   # stands for a non-NULL, 16-byte aligned pointer: validation comes before any launch


def _pca_normals(xyz, off, K):
    idx = so.knn(xyz, off, K)
    return normals_oracle.frames(xyz, K, idx=idx.astype(np.int64), dtype=np.float64, disambiguate=False)["normals"].astype(np.float32), idx


# ---------------------------------------------------------------- the oracle checks itself
@pytest.fixture(scope="module")
def sphere():
    """600 points on the unit sphere, analytic normals with random signs, K = 12"""
    xyz, ana = so.ellipsoid(600, 7, axes=(1.0, 1.0, 1.0))
    off = np.array([600], np.int32)
    signs = np.random.default_rng(8).choice([-1.0, 1.0], 600)
    normals = (ana * signs[:, None]).astype(np.float32)
    idx = so.knn(xyz, off, 12)
    return xyz, ana, normals, idx, off, so.orient(xyz, normals, idx, off)


def test_oracle_forest_is_a_minimum_spanning_tree(sphere):
    """total weight against scipy's on the same graph; the integer weights 1 + (fp32 bits of w >> 8) are exact in fp64 and keep
    scipy from dropping an edge of weight 0"""
    _, _, _, _, _, o = sphere
    u, v, key, wb, _ = o["edges"]
    assert len(np.unique(key)) == len(key) and (np.diff(key.astype(np.uint64)) > 0).all()      # a strict total order
    g = coo_matrix(((wb + 1).astype(np.float64), (u, v)), shape=(600, 600))
    ncomp, _ = connected_components(g, directed=False)
    assert len(o["forest"]) == 600 - ncomp == 599
    assert int(minimum_spanning_tree(g).sum()) == int((wb[o["forest"]] + 1).sum())


def test_oracle_sphere_comes_out_all_outward(sphere):
    xyz, ana, normals, _, _, o = sphere
    side = (o["oriented"].astype(np.float64) * ana).sum(1)
    assert (side > 0).all() or (side < 0).all()
    assert (side > 0).all()                                   # the root rule: the top of a sphere has n_z > 0 outward
    assert np.array_equal(np.abs(o["oriented"]), np.abs(normals)) and set(np.unique(o["signs"])) == {-1, 1}
    assert (o["comp"] == 0).all()


def test_oracle_result_does_not_depend_on_the_input_signs(sphere):
    xyz, _, normals, idx, off, o = sphere
    rng = np.random.default_rng(9)
    for _ in range(3):
        flip = rng.random(600) < 0.5
        again = so.orient(xyz, np.where(flip[:, None], -normals, normals), idx, off)
        assert np.array_equal(again["oriented"].view(np.uint32), o["oriented"].view(np.uint32))
        assert np.array_equal(again["signs"], np.where(flip, -o["signs"], o["signs"]))


def test_oracle_segments_and_short_segments():
    """segments are oriented on their own; k_s = min(K, n_s - 1) columns, so two points have no edge and stay two components"""
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(40, 3)).astype(np.float32)
    normals = (rng.integers(-4, 5, (40, 3)) / 8).astype(np.float32)
    normals[(normals == 0).all(1)] = [0.5, 0, 0]
    off = np.array([30, 32, 33, 33, 40], np.int32)
    idx = so.knn(xyz, off, 8)
    o = so.orient(xyz, normals, idx, off)
    assert o["comp"][30] == 30 and o["comp"][31] == 31 and o["comp"][32] == 32            # n_s = 2 and n_s = 1: no edges
    assert o["signs"][32] == (-1 if normals[32, 2] < 0 else 1)
    assert (o["comp"][:30] < 30).all() and (o["comp"][33:] >= 33).all()
    alone = so.orient(xyz[33:], normals[33:], idx[33:] - 33, np.array([7], np.int32))
    assert np.array_equal(alone["signs"], o["signs"][33:]) and np.array_equal(alone["comp"] + 33, o["comp"][33:])


def test_oracle_clusters_by_hand():
    """two disjoint tetrahedra plus two triangles sharing only a vertex: 4 clusters; a fan of three faces on one edge: one"""
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    faces = np.concatenate([tet, tet + 4, [[8, 9, 10], [8, 11, 12]]])
    clusters, c = so.face_clusters(faces)
    assert c == 4 and clusters.tolist() == [0] * 4 + [1] * 4 + [2, 3]
    verts, fan = so.fan_mesh()
    clusters, c = so.face_clusters(fan)
    assert c == 4 and clusters.tolist() == [0, 1, 0, 2, 0, 3]                             # numbered by their smallest face
    area, num, vsum = so.cluster_stats(verts, fan, clusters)
    assert num.tolist() == [5, 3, 3, 3]                                                   # vertex 5 counts in clusters 1 and 3
    np.testing.assert_allclose(area[2], 0.5, rtol=0, atol=1e-15)
    np.testing.assert_allclose(vsum[1], [17, 0, 0], rtol=0, atol=1e-15)


def test_oracle_keep_and_compact_by_hand():
    verts = np.array([[0.5, 0.5, 0.5], [3.0, 1.0, 1.0], [1.0, 3.9, 1.0], [9.5, 1.0, 1.0], [-0.2, 1.0, 1.0], [1.0, 1.0, 2.0]], np.float32)
    mask = np.zeros((3, 4, 5), bool)                                                      # D, H, W: z < 3, y < 4, x < 5
    mask[:, :, :] = True
    mask[0, 0, 0] = False
    keep = so.keep_flags(verts, mask=mask, spacing=(2.0, 1.0, 1.0))
    # vertex 0 falls into the cleared voxel; 3 is beyond the volume in x and clamps to x = 4 (set); 4 is negative: dropped
    assert keep.tolist() == [False, True, True, True, False, True]
    keep = so.keep_flags(verts, box=[[0.5, 0.5, 0.5], [3.0, 3.9, 2.0]])
    assert keep.tolist() == [True, True, True, False, False, True]                       # on the box faces: kept
    faces = np.array([[1, 2, 5], [0, 1, 2], [1, 5, 3]])
    v, f = so.compact(verts, faces, np.array([0, 1, 1, 1, 1, 1], bool))
    assert len(v) == 5 and f.tolist() == [[0, 1, 4], [0, 4, 2]]
    v, f = so.compact(verts, faces, np.array([0, 1, 1, 1, 1, 1], bool), np.array([1, 1, 0], bool), True)
    assert np.array_equal(v, verts[[1, 2, 5]]) and f.tolist() == [[0, 1, 2]]
    v, f = so.compact(verts, faces, np.zeros(6, bool), None, True)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_oracle_biggest_component_rule():
    """three squares of area 4, 9, 1 at x = 0, 10, 20: the -1 / area rule"""
    def square(x0, s, base):
        v = np.array([[x0, 0, 0], [x0 + s, 0, 0], [x0 + s, s, 0], [x0, s, 0]], np.float64)
        return v, np.array([[0, 1, 2], [0, 2, 3]]) + base
    parts = [square(0, 2, 0), square(10, 3, 4), square(20, 1, 8)]
    verts, faces = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert so.biggest_component(verts, faces)[0] == 1
    assert so.biggest_component(verts, faces, right=True, center_x=5.0)[0] == 0          # right: the mean has to be <= center_x
    assert so.biggest_component(verts, faces, right=False, center_x=15.0)[0] == 2
    assert so.biggest_component(verts, faces, right=True, center_x=None)[0] == 1
    # nothing on the wanted side: -1 / area is largest for the biggest
    assert so.biggest_component(verts, faces, right=True, center_x=-1.0)[0] == 1
    assert so.biggest_component(verts, faces, right=False, center_x=30.0)[0] == 1


def test_oracle_fixture_has_the_cases_the_gpu_test_needs():
    """the blob field: four blobs, two of them meeting at one cell; marching cubes (the fp64 oracle's) gives closed pieces"""
    f = so.blob_field()
    assert f.shape == so.FIELD_SHAPE and f.dtype == np.float32
    assert f[18, 4, 22] < 0 and f[19, 5, 23] < 0 and f[18, 5, 23] > 0 and f[19, 4, 22] > 0
    v, faces, _ = mc_oracle.marching_cubes_item(f, 0.0, False, None, np.float64)
    clusters, c = so.face_clusters(faces)
    assert c in (4, 5) and mc_oracle.directed_edge_defect(faces)[0] == 0
    area, num, _ = so.cluster_stats(v, faces, clusters)
    assert (area > 10).all() and (num > 20).all()


def test_oracle_distance_to_an_ellipsoid():
    axes = np.array([3.0, 2.0, 1.0])
    p = np.array([[5.0, 0, 0], [0, 0, 0.25], [0, -4.0, 0], [3.0, 0, 0], [1e-9, 1e-9, 3.0]])
    np.testing.assert_allclose(so.ellipsoid_distance(p, axes), [2.0, 0.75, 2.0, 0.0, 2.0], rtol=0, atol=1e-7)
    on, _ = so.ellipsoid(50, 4)
    assert so.ellipsoid_distance(on.astype(np.float64) * 10 + [1, 2, 3], np.array(so.AXES) * 10, (1, 2, 3)).max() < 1e-5


@pytest.mark.parametrize("cloud", ["ellipsoid", "sheet"])
def test_seeded_clouds_meet_the_precondition_of_the_gpu_tests(cloud):
    """2048 points, PCA normals (fp64 oracle, no disambiguation), K = 16: the graph is ONE component and the oriented normals
    agree with the analytic ones everywhere -- a property of the seeds and of the method, shown here without any kernel"""
    xyz, ana = so.ellipsoid(2048, 1) if cloud == "ellipsoid" else so.wavy_sheet(2048, 1)
    off = np.array([2048], np.int32)
    normals, idx = _pca_normals(xyz, off, 16)
    o = so.orient(xyz, normals, idx, off)
    assert (o["comp"] == 0).all()
    assert ((o["oriented"].astype(np.float64) * ana).sum(1) > 0).all()
    assert 100 < (o["signs"] < 0).sum() < 1948                # the PCA signs really are arbitrary


# ---------------------------------------------------------------- the C ABI
def test_symbols_declared_bound_and_exported():
    from fissure_segmentation_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    declared = set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    csrc = os.path.join(ROOT, "fissure-segmentation_amd", "csrc")
    assert "mesh_cleanup.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert '#include "fsg_common.h"' in open(os.path.join(csrc, "mesh_cleanup.hip")).read()


def test_orient_workspace_query():
    from fissure_segmentation_amd import _lib
    q = _lib.lib.fsg_orient_normals_workspace_bytes
    assert q(0, 8) == 0 and q((1 << 20) + 1, 8) == 0
    for n in (1, 2, 257, 20000, 1 << 20):
        assert q(n, 8) >= 36 * n and q(n, 8) % 16 == 0 and q(n, 8) == q(n, 64)


def _call(name, *args):
    from fissure_segmentation_amd import _lib
    _lib.call(name, *args)


def test_bad_arguments_are_reported_before_launch():
    orient = lambda **kw: _call("fsg_orient_normals_f32", *[kw.get(k, d) for k, d in (       # noqa: E731
        ("xyz", P), ("normals", P), ("idx", P), ("offset", P), ("b", 1), ("n", 10), ("K", 8), ("ws", P), ("ws_bytes", 1 << 20),
        ("out", P), ("signs", P), ("comp", P))], None)
    for null in ("xyz", "normals", "idx", "offset", "out", "signs", "comp"):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            orient(**{null: None})
    for bad in ({"b": 0}, {"n": -1}, {"K": 1}, {"K": 65}):
        with pytest.raises(RuntimeError, match="bad shape"):
            orient(**bad)
    with pytest.raises(RuntimeError, match="20 bits per endpoint"):
        orient(n=(1 << 20) + 1)
    for bad in ({"ws": None}, {"ws": 8}, {"ws_bytes": 100}):
        with pytest.raises(RuntimeError, match="workspace"):
            orient(**bad)
    orient(n=0, ws=None, ws_bytes=0)                          # nothing to do, nothing launched

    with pytest.raises(RuntimeError, match="NULL pointer"):
        _call("fsg_face_union_i32", None, P, 4, P, P, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _call("fsg_face_union_i32", P, P, 4, P, None, None)
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("fsg_face_union_i32", P, P, -1, P, P, None)
    _call("fsg_face_union_i32", P, P, 0, P, P, None)

    stats = [P, P, P, P, P, 8, 4, 2, P, P, P, None]
    for i in (0, 1, 2, 3, 4, 8, 9, 10):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            _call("fsg_cluster_stats_f64", *[None if j == i else a for j, a in enumerate(stats)])
    for i, bad in ((5, 0), (6, 0), (7, -1), (7, 5)):
        with pytest.raises(RuntimeError, match="bad shape"):
            _call("fsg_cluster_stats_f64", *[bad if j == i else a for j, a in enumerate(stats)])

    keep = [P, 8, P, 1, None, None, None, 0, 0, 0, 1.0, 1.0, 1.0, P, None]
    for i in (0, 2, 13):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            _call("fsg_mesh_keep_flags_u8", *[None if j == i else a for j, a in enumerate(keep)])
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("fsg_mesh_keep_flags_u8", *[0 if j == 3 else a for j, a in enumerate(keep)])
    masked = [P if j == 6 else a for j, a in enumerate(keep)]
    with pytest.raises(RuntimeError, match="bad mask volume"):
        _call("fsg_mesh_keep_flags_u8", *masked)
    masked[7:10] = [4, 4, 4]
    for s in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        with pytest.raises(RuntimeError, match="spacing"):
            _call("fsg_mesh_keep_flags_u8", *masked[:10], *s, P, None)

    with pytest.raises(RuntimeError, match="NULL pointer"):
        _call("fsg_mesh_face_flags_u8", None, 8, 4, P, None, P, P, None)
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("fsg_mesh_face_flags_u8", P, 0, 4, P, None, P, P, None)
    compact = [P, None, P, 8, 4, P, 1, P, P, P, P, P, None, P, None]
    for i in (0, 2, 5, 7, 8, 9, 10, 11, 13):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            _call("fsg_mesh_compact_f32", *[None if j == i else a for j, a in enumerate(compact)])
    with pytest.raises(RuntimeError, match="normals in and out"):
        _call("fsg_mesh_compact_f32", *[P if j == 1 else a for j, a in enumerate(compact)])
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("fsg_mesh_compact_f32", *[0 if j == 3 else a for j, a in enumerate(compact)])


# ---------------------------------------------------------------- the host-side contract
def test_surface_fitting_argument_errors_need_no_gpu():
    from fissure_segmentation_amd.data_processing import pointcloud_surface_fitting as sf
    with pytest.raises(ValueError, match="Tried reconstructing mesh from 3 points. Requires at least 4."):
        sf.pointcloud_surface_fitting(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="from 0 points"):
        sf.pointcloud_surface_fitting(torch.zeros(0, 3))
    pts = np.random.default_rng(0).normal(size=(10, 3)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="width"):
        sf.pointcloud_surface_fitting(pts, width=1)
    with pytest.raises(NotImplementedError, match="depth"):
        sf.pointcloud_surface_fitting(pts, depth=9)
    with pytest.raises(ValueError, match="spacing"):
        sf.pointcloud_surface_fitting(pts, mask=np.ones((4, 4, 4), bool))
    with pytest.raises(NotImplementedError, match="width"):
        sf.fit_label_surfaces(pts, np.ones(10, np.int64), 2, width=2)
    assert not hasattr(sf, "poisson_reconstruction") and not hasattr(sf, "regularize_fissure_segmentations")
    from fissure_segmentation_amd.data_processing import surface_fitting as label_maps
    assert not hasattr(label_maps, "pointcloud_surface_fitting") and hasattr(label_maps, "o3d_mesh_to_labelmap")


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import fissure_segmentation_amd as fsg
    from fissure_segmentation_amd.mesh import Meshes
    from fissure_segmentation_amd.utils import general_utils as gu
    F = fsg.functional
    xyz, nr, off = torch.rand(10, 3), torch.rand(10, 3), torch.tensor([10])
    with pytest.raises(RuntimeError, match="GPU"):
        F.orient_normals_consistent(xyz, nr, off, 4)
    with pytest.raises(ValueError, match="neighborhood_size"):
        F.orient_normals_consistent(xyz, nr, off, 65)
    with pytest.raises(ValueError, match="shape of xyz"):
        F.orient_normals_consistent(xyz, nr[:5], off, 4)
    with pytest.raises(ValueError, match="offset"):
        F.orient_normals_consistent(xyz, nr, off.float(), 4)
    with pytest.raises(ValueError, match="at most"):
        F.orient_normals_consistent(torch.empty((1 << 20) + 1, 3), torch.empty((1 << 20) + 1, 3), off, 4)
    verts, faces = torch.tensor([[0., 0, 0], [2, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]])
    m = Meshes([verts], [faces])
    for call in (lambda: F.mesh_face_components(m), lambda: F.mesh_component_stats(m, torch.zeros(1, dtype=torch.int32)),
                 lambda: F.mesh_remove_vertices(m), lambda: gu.remove_all_but_biggest_component(m),
                 lambda: gu.mask_out_verts_from_mesh(m, torch.ones(2, 2, 2, dtype=torch.bool), (1., 1., 1.))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="Meshes"):
        F.mesh_face_components(verts)
    with pytest.raises(ValueError, match="integer vertex indices"):
        F.mesh_face_components((verts, faces.float()))
    empty = Meshes([verts[:0]], [faces[:0]])
    assert gu.remove_all_but_biggest_component(empty) is empty                          # the reference's early return


def test_aliases():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from data_processing.surface_fitting import pointcloud_surface_fitting
        from utils.general_utils import mask_out_verts_from_mesh, remove_all_but_biggest_component   # noqa: F401
        from data_processing.surface_fitting import o3d_mesh_to_labelmap
        assert pointcloud_surface_fitting.__module__ == "fissure_segmentation_amd.data_processing.pointcloud_surface_fitting"
        assert o3d_mesh_to_labelmap.__module__ == "fissure_segmentation_amd.data_processing.surface_fitting"
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
