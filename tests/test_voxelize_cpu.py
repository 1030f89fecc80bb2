"""CPU tests of the mesh -> label map feature (csrc/voxelize.hip, functional.mesh_labelmap_dist / mesh_labelmap_cover and
the reference-named wrappers): the C ABI's declarations and host-side argument checks, the fp64 oracle of
tests/voxelize_oracle.py against cases worked out by hand -- it is what the kernels are held to on the GPU --, the plain-torch
helpers against the real reference's recorded outputs, and the host-side contract (imports without a GPU, refuses CPU
tensors)."""
import os
import re

import numpy as np
import pytest
import torch

import voxelize_oracle as vo
from conftest import ROOT
from golden_util import load

NEW_SYMBOLS = ("fsg_mesh_labelmap_dist_f32", "fsg_mesh_labelmap_cover_f32")
P = 8   # stands for a non-NULL pointer: validation comes before any launch


def test_symbols_declared_bound_and_exported():
    from fissure_segmentation_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    declared = set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    csrc = os.path.join(ROOT, "fissure-segmentation_amd", "csrc")
    assert "voxelize.hip" in open(os.path.join(csrc, "Makefile")).read()
    # the point-triangle arithmetic exists once, in the header both kernels include
    for name in ("point_mesh.hip", "voxelize.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "point_face.h"' in text and "void face_record(" not in text and "float point_face(" not in text, name


def _dist(*, verts=P, faces=P, labels=P, V=3, F=1, shape=(4, 4, 4), spacing=(1., 1., 1.), thr=1.0, mask=None, keys=P, out=P):
    from fissure_segmentation_amd import _lib
    _lib.call("fsg_mesh_labelmap_dist_f32", verts, faces, labels, V, F, *shape, *spacing, thr, mask, keys, out, None)


def _cover(*, verts=P, faces=P, labels=P, V=3, F=1, shape=(4, 4, 4), spacing=(1., 1., 1.), out=P):
    from fissure_segmentation_amd import _lib
    _lib.call("fsg_mesh_labelmap_cover_f32", verts, faces, labels, V, F, *shape, *spacing, out, None)


@pytest.mark.parametrize("entry", [_dist, _cover], ids=["dist", "cover"])
def test_bad_arguments_are_reported_before_launch(entry):
    for null in ("verts", "faces", "labels", "out"):
        with pytest.raises(RuntimeError, match="NULL pointer"):
            entry(**{null: None})
    for bad in ({"V": 0}, {"F": 0}, {"F": -1}, {"shape": (0, 4, 4)}, {"shape": (4, -1, 4)}, {"shape": (4, 4, 0)}):
        with pytest.raises(RuntimeError, match="bad shape"):
            entry(**bad)
    for s in ((0., 1., 1.), (1., -1., 1.), (1., 1., float("nan")), (float("inf"), 1., 1.)):
        with pytest.raises(RuntimeError, match="spacing"):
            entry(spacing=s)
    for shape in ((2048, 1024, 1024), (1, 1 << 16, 1 << 15), (1290, 1290, 1291)):      # 2^31 and just above
        with pytest.raises(RuntimeError, match="2\\^31 voxels"):
            entry(shape=shape)


def test_dist_threshold_and_key_volume_are_checked():
    with pytest.raises(RuntimeError, match="negative or NaN"):
        _dist(thr=-1e-3)
    with pytest.raises(RuntimeError, match="negative or NaN"):
        _dist(thr=float("nan"))
    with pytest.raises(RuntimeError, match="key volume"):
        _dist(keys=None)


# ---------------------------------------------------------------- the oracle against cases worked out by hand
def test_oracle_band_of_an_axis_aligned_triangle_is_a_slab():
    """a right triangle in the plane x0 = 2.6 of a volume with spacing (1.25, 0.5, 1): above its interior the distance is
    |i0 * 1.25 - 2.6|, so with threshold 1.0 exactly the planes i0 = 2 (0.1) and i0 = 3 (1.15 > 1: not) ... by hand:
    i0 = 2 -> 0.1, i0 = 1 -> 1.35, i0 = 3 -> 1.15; threshold 1.2 takes i0 in {2, 3}"""
    shape, spacing = (6, 12, 8), (1.25, 0.5, 1.0)
    verts = np.array([[2.6, -20., -20.], [2.6, 60., -20.], [2.6, -20., 60.]])     # covers the whole cross-section
    dist = vo.distances([(verts, np.array([[0, 1, 2]]))], shape, spacing)
    i0 = np.arange(6)[:, None, None] * np.ones(shape)
    np.testing.assert_allclose(dist[0].reshape(shape), np.abs(i0 * 1.25 - 2.6), rtol=0, atol=1e-12)
    for thr, planes in ((1.0, [2]), (1.2, [2, 3]), (0.05, []), (1.4, [1, 2, 3])):
        want = np.zeros(shape, dtype=np.int64)
        want[planes] = 1
        assert np.array_equal(vo.labelmap_dist(dist, shape, thr), want), thr
        assert vo.check_dist(want, dist, shape, thr)[1:3] == (0, 0)
    # a threshold within the tolerance of a plane's distance excuses that plane: it may be labelled or not
    assert vo.check_dist(np.zeros(shape, dtype=np.int64), dist, shape, 0.1 + 1e-4)[1:3] == (96, 0)
    # a small triangle: the band is the slab over the triangle plus the rounded rim, here only its voxel count by hand:
    # the triangle (1, 1, 1) (1, 3, 1) (1, 1, 4) in a unit grid, threshold 0: exactly the lattice points on it
    tri = np.array([[1., 1., 1.], [1., 3., 1.], [1., 1., 4.]])
    d = vo.distances([(tri, np.array([[0, 1, 2]]))], (3, 5, 6), (1., 1., 1.))
    on = vo.labelmap_dist(d, (3, 5, 6), 0.0)
    # lattice points with i0 = 1, i1 >= 1, i2 >= 1 and (i1 - 1) / 2 + (i2 - 1) / 3 <= 1
    want = {(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (1, 2, 1), (1, 2, 2), (1, 3, 1)}
    assert set(map(tuple, np.argwhere(on == 1))) == want


def test_oracle_ties_and_masks():
    """two parallel planes at equal distance from the plane of voxels between them: the lower mesh wins, both are allowed"""
    shape, spacing = (5, 4, 4), (1., 1., 1.)
    big = np.array([[0., -20., -20.], [0., 60., -20.], [0., -20., 60.]])
    meshes = [(big + [3., 0, 0], np.array([[0, 1, 2]])), (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)),
              (big + [1., 0, 0], np.array([[0, 1, 2]]))]
    dist = vo.distances(meshes, shape, spacing)
    assert np.isinf(dist[1]).all()
    want = vo.labelmap_dist(dist, shape, 1.0)
    assert [int(want[i, 0, 0]) for i in range(5)] == [3, 3, 1, 1, 1]              # i0 = 2: tie, lowest mesh; the empty mesh keeps its number
    labelled, excused, wrong, where = vo.check_dist(want, dist, shape, 1.0)
    assert (labelled, wrong) == (80, 0) and where[2].all() and where[0].all() and where[4].all() and not where[1].any()
    swapped = want.copy()
    swapped[2] = 3                                                                 # the other side of the tie is allowed
    assert vo.check_dist(swapped, dist, shape, 1.0)[2] == 0
    swapped[1] = 1                                                                 # a wrong label is not
    assert vo.check_dist(swapped, dist, shape, 1.0)[2] == 16
    mask = np.zeros(shape, dtype=bool)
    mask[:, :2] = True
    assert np.array_equal(vo.labelmap_dist(dist, shape, 1.0, mask), np.where(mask, want, 0))
    assert vo.check_dist(want, dist, shape, 1.0, mask)[2] == 40                   # labels outside the mask are wrong


def test_oracle_triangle_exactly_on_a_cell_face():
    """floor(x / s) puts a triangle in the plane x0 = 3 s0 into the cells i0 = 3, not i0 = 2; the closed test meets both"""
    shape, spacing = (6, 4, 4), (1.25, 0.5, 1.0)                                  # binary fractions: cell limits are exact
    verts = np.array([[3.75, 0.25, 0.5], [3.75, 1.25, 0.5], [3.75, 0.25, 2.5]])
    faces = np.array([[0, 1, 2]])
    exact = vo.cover_hits(verts, faces, shape, spacing)
    assert set(np.argwhere(exact)[:, 0]) == {3}
    # in the plane: cells i1 = 0..2 (0.25 .. 1.25 -> floor(./0.5) = 0, 1, 2), i2 = 0..2, minus those beyond the hypotenuse
    want = {(3, 0, 0), (3, 0, 1), (3, 0, 2), (3, 1, 0), (3, 1, 1), (3, 2, 0), (3, 1, 2), (3, 2, 1)}
    # hypotenuse from (1.25, 0.5) to (0.25, 2.5): cell (i1=1, i2=2) = [0.5,1) x [2,3) contains (0.5, 2) which is inside
    # (0.5 - 0.25) / 1 + (2 - 0.5) / 2 = 1.0 <= 1; cell (2, 1) = [1,1.5) x [1,2) contains (1, 1): 0.75 + 0.25 = 1.0 <= 1; (2, 2) has
    # its nearest corner (1, 2) at 0.75 + 0.75 > 1: outside
    assert set(map(tuple, np.argwhere(exact))) == want
    grown = vo.cover_hits(verts, faces, shape, spacing, vo.COVER_TOL)
    shrunk = vo.cover_hits(verts, faces, shape, spacing, -vo.COVER_TOL)
    assert set(np.argwhere(grown)[:, 0]) == {2, 3} and not shrunk.any()
    assert vo.check_cover(exact.astype(np.int64), [(shrunk, grown)]) == (0, int(grown.sum()), 0)


def test_oracle_box_test_by_hand():
    centre, half = np.array([[0.5, 0.5, 0.5]]), np.array([0.5, 0.5, 0.5])
    tri = np.array([[[2., -1, -1], [-1, 2, -1], [-1, -1, 2]],        # x + y + z = 0 ... cuts the unit cube's corner region: hits
                    [[4., 0, 0], [0, 4, 0], [0, 0, 4]],              # x + y + z = 4 > 3: only the normal separates
                    [[1.2, -5, 0.5], [1.2, 5, 0.5], [5, 0, 0.5]],    # beyond x = 1: a box axis separates
                    [[1.5, 0.7, 0.5], [0.7, 1.5, 0.5], [1.6, 1.6, 0.5]],   # in the plane z = 0.5, beyond x + y = 2.2: only an edge axis separates
                    [[0.2, 0.2, 0.2], [0.9, 0.9, 0.9], [0.55, 0.55, 0.55]],   # no area, inside: its longest edge
                    [[1.5, -0.2, 0.5], [-0.2, 1.5, 0.5], [0.65, 0.65, 0.5]],  # no area, crossing: x + y = 1.3 passes through
                    [[2.5, -0.2, 0.5], [-0.2, 2.5, 0.5], [1.15, 1.15, 0.5]],  # no area, x + y = 2.3 misses the corner (1, 1)
                    [[0.4, 0.4, 0.4]] * 3, [[1.4, 0.4, 0.4]] * 3])           # points
    assert vo.tri_box_overlap(tri, centre, half)[0].tolist() == [True, False, False, False, True, True, False, True, False]
    # half-open: a point on the upper face is out, on the lower face in
    pts = np.array([[[1.0, 0.5, 0.5]] * 3, [[0.0, 0.5, 0.5]] * 3])
    assert vo.tri_box_overlap(pts, centre, half).tolist() == [[True, True]]
    assert vo.tri_box_overlap(pts, centre, half, half_open=True).tolist() == [[False, True]]
    assert vo.tri_box_overlap(tri[:1], centre, half - 0.51).tolist() == [[False]]   # the half size is an argument


def test_oracle_sampling_restatement_stays_inside_the_exact_cover():
    meshes = [vo.sheet(*vo.SHEETS[2])]
    exact = vo.cover_hits(*meshes[0], vo.SHAPE, vo.SPACING)
    sampled = vo.sampled_labelmap(meshes, vo.SHAPE, vo.SPACING, n=20_000)
    assert sampled.max() == 1 and not ((sampled != 0) & ~exact).any()
    assert 0.5 * exact.sum() < (sampled != 0).sum() <= exact.sum()


def test_seeded_inputs_meet_the_precondition_of_the_gpu_tests():
    """the voxels / cells that the rules excuse are at most 1 % of the labelled ones -- a property of the seeded sheets and of
    the oracle, checked here without any kernel, so that on the GPU the excusal cannot hide much"""
    meshes = vo.sheets()
    assert [len(f) for _, f in meshes] == [200, 200, 200]
    for v, _ in meshes:                                                           # they leave the volume on all sides of axes 1, 2
        assert v[:, 1].min() < 0 and v[:, 2].min() < 0 and v[:, 1].max() > vo.extent()[1] and v[:, 2].max() > vo.extent()[2]
    dist = vo.distances(meshes, vo.SHAPE, vo.SPACING)
    for thr in (1.0, 1.5):
        for mask in (None, vo.random_mask()):
            labelled, excused, wrong, _ = vo.check_dist(vo.labelmap_dist(dist, vo.SHAPE, thr, mask), dist, vo.SHAPE, thr, mask)
            assert wrong == 0 and labelled > 1000 and excused <= vo.EXCUSED_SHARE * labelled, (thr, labelled, excused)
    bounds = vo.cover_bounds(meshes, vo.SHAPE, vo.SPACING)
    figures = [(int(must.sum()), int((must != may).sum())) for must, may in bounds]
    assert figures == [(1129, 10), (1234, 3), (804, 3)]
    assert all(excused <= vo.EXCUSED_SHARE * labelled for labelled, excused in figures)
    exact = np.zeros(vo.SHAPE, dtype=np.int64)
    for m, (v, f) in enumerate(meshes):
        exact[vo.cover_hits(v, f, vo.SHAPE, vo.SPACING)] = m + 1
    labelled, excused, wrong = vo.check_cover(exact, bounds)
    assert wrong == 0 and excused <= vo.EXCUSED_SHARE * labelled


# ---------------------------------------------------------------- plain torch helpers against the reference's outputs
def test_mask_to_points_and_points_to_label_map_match_the_reference():
    from fissure_segmentation_amd.utils import general_utils as gu
    g = load("voxelize_ref")
    assert int(g["util_seed"]) == vo.UTIL_SEED
    mask, pts, labels = vo.util_inputs()
    got = gu.mask_to_points(torch.from_numpy(mask), vo.UTIL_SPACING_XYZ)
    assert got.dtype == torch.float32 and got.shape == (int(mask.sum()), 3)
    assert np.array_equal(got.numpy(), g["mask_to_points"])
    lm, idx = gu.points_to_label_map(torch.from_numpy(pts), torch.from_numpy(labels), vo.UTIL_SHAPE, vo.UTIL_SPACING_XYZ)
    assert lm.dtype == torch.int64 and tuple(lm.shape) == vo.UTIL_SHAPE and idx.dtype == torch.int64
    assert np.array_equal(idx.numpy(), g["points_index"]) and np.array_equal(lm.numpy(), g["points_label_map"])
    assert len(np.unique(g["points_index"], axis=0)) == len(pts)                  # one point per voxel: no scatter order involved
    assert (g["points_index"][:3] == [[0, 1, 1], [5, 2, 0], [1, 6, 4]]).all()     # the three outside points were clamped


def test_reference_recordings_agree_with_the_oracle():
    """what the real reference's mesh2labelmap_dist makes of fp64 oracle distances IS the oracle's label map, and what its
    o3d_mesh_to_labelmap scatters lies inside the exact cover"""
    g = load("voxelize_ref")
    assert bool(g["have_dist"]) and bool(g["have_o3d"])
    assert int(g["sample_seed"]) == vo.SAMPLE_SEED and int(g["n_samples"]) == vo.N_SAMPLES
    sampled = vo.sampled_labelmap(vo.sheets(), vo.SHAPE, vo.SPACING)
    assert np.array_equal(g["o3d_all"], sampled)      # the restatement: floor == truncation once negative samples are left out


def test_host_contract_without_a_gpu():
    import fissure_segmentation_amd as fsg
    from fissure_segmentation_amd import metrics
    from fissure_segmentation_amd.data_processing import surface_fitting as sf, surface_fitting_optimization as sfo
    assert hasattr(metrics, "label_mesh_assd") and not hasattr(metrics, "label_label_assd")
    for mod, absent in ((sf, ("poisson_reconstruction", "pointcloud_surface_fitting", "regularize_fissure_segmentations")),
                        (sfo, ("fit_plane_to_fissure", "Plane"))):
        assert not any(hasattr(mod, n) for n in absent)
    verts, faces = torch.tensor([[0., 0, 0], [2, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="GPU"):
        fsg.functional.mesh_labelmap_dist([verts], [faces], (4, 4, 4), (1., 1., 1.))
    with pytest.raises(RuntimeError, match="GPU"):
        fsg.functional.mesh_labelmap_cover([verts], [faces], (4, 4, 4), (1., 1., 1.))
    with pytest.raises(RuntimeError, match="GPU"):
        sfo.mesh2labelmap_dist([(verts, faces)], (4, 4, 4), (1., 1., 1.))
    with pytest.raises(RuntimeError, match="GPU"):
        sf.mesh2labelmap_sampling([(verts, faces)], (4, 4, 4), (1., 1., 1.))
    with pytest.raises(RuntimeError, match="GPU"):
        sf.o3d_mesh_to_labelmap([(verts, faces)], (4, 4, 4), (1., 1., 1.))
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.label_mesh_assd(torch.ones(2, 2, 2), (verts, faces))


def test_aliases():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from data_processing.surface_fitting import mesh2labelmap_sampling, o3d_mesh_to_labelmap   # noqa: F401
        from data_processing.surface_fitting_optimization import mesh2labelmap_dist
        from utils.general_utils import mask_to_points, points_to_label_map                      # noqa: F401
        assert mesh2labelmap_dist.__module__ == "fissure_segmentation_amd.data_processing.surface_fitting_optimization"
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
