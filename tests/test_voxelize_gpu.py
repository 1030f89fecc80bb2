"""GPU tests of the mesh -> label map kernels (csrc/voxelize.hip) and their wrappers against the fp64 oracle of
tests/voxelize_oracle.py, which tests/test_voxelize_cpu.py pins by hand, and against what the real reference recorded
(tests/golden/voxelize_ref.npz).

The rules (voxelize_oracle.check_dist / check_cover): a distance label map must equal the oracle's except where the fp64
distance is within 1e-3 mm of the threshold (0 or the label) or two meshes are within 1e-3 mm of each other (either label); a
coverage map must label every cell hit with the cell shrunk by 1e-3 per side and none missed with the cell grown by 1e-3.  On
the seeded sheets the excused voxels may be at most 1 % of the oracle's labelled ones.  Every case prints its figures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import voxelize_oracle as vo
from golden_util import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ref():
    """everything the oracle says about the three sheets, computed once and only read"""
    meshes = vo.sheets()
    return SimpleNamespace(meshes=meshes, dist=vo.distances(meshes, vo.SHAPE, vo.SPACING), mask=vo.random_mask(),
                           bounds=vo.cover_bounds(meshes, vo.SHAPE, vo.SPACING),
                           sampled=[vo.sampled_labelmap([m], vo.SHAPE, vo.SPACING, seed=vo.SAMPLE_SEED + i) for i, m in enumerate(meshes)],
                           sampled_all=vo.sampled_labelmap(meshes, vo.SHAPE, vo.SPACING), golden=load("voxelize_ref"))


def G(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def split(meshes, device):
    return [G(v, device, torch.float32) for v, _ in meshes], [G(f, device) for _, f in meshes]


def run_dist(fsg, device, meshes, shape, spacing, thr, mask=None):
    verts, faces = split(meshes, device)
    m = None if mask is None else G(mask, device)
    out = fsg.functional.mesh_labelmap_dist(verts, faces, shape, spacing, thr, m)
    assert out.dtype == torch.int64 and out.device == device and tuple(out.shape) == tuple(shape)
    again = fsg.functional.mesh_labelmap_dist(verts, faces, shape, spacing, thr, m)
    assert torch.equal(out, again)
    return N(out)


def run_cover(fsg, device, meshes, shape, spacing):
    verts, faces = split(meshes, device)
    out = fsg.functional.mesh_labelmap_cover(verts, faces, shape, spacing)
    assert out.dtype == torch.int64 and out.device == device and tuple(out.shape) == tuple(shape)
    assert torch.equal(out, fsg.functional.mesh_labelmap_cover(verts, faces, shape, spacing))
    return N(out)


# ---------------------------------------------------------------- the seeded sheets
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("thr", [1.0, 1.5])
def test_distance_map_vs_fp64_oracle(fsg, device, ref, thr, masked):
    mask = ref.mask if masked else None
    got = run_dist(fsg, device, ref.meshes, vo.SHAPE, vo.SPACING, thr, mask)
    labelled, excused, wrong, where = vo.check_dist(got, ref.dist, vo.SHAPE, thr, mask)
    differ = int((got != vo.labelmap_dist(ref.dist, vo.SHAPE, thr, mask)).sum())
    print(f"dist thr={thr} masked={masked}: labelled {labelled} excused {excused} used {differ} wrong {wrong}")
    assert labelled > 1000 and wrong == 0
    assert excused <= vo.EXCUSED_SHARE * labelled
    recorded = ref.golden[f"dist_{thr}" + ("_mask" if masked else "")]             # the real reference on oracle distances
    assert not ((got != recorded) & ~where).any()


@pytest.mark.parametrize("which", [0, 1, 2, "all"])
def test_coverage_map_vs_fp64_oracle(fsg, device, ref, which):
    pick = [0, 1, 2] if which == "all" else [which]
    got = run_cover(fsg, device, [ref.meshes[i] for i in pick], vo.SHAPE, vo.SPACING)
    bounds = [ref.bounds[i] for i in pick]
    labelled, excused, wrong = vo.check_cover(got, bounds)
    print(f"cover {which}: labelled {labelled} excused {excused} wrong {wrong}")
    assert labelled > 500 and wrong == 0
    assert excused <= vo.EXCUSED_SHARE * labelled
    # the reference's route, restated: what 2 10^5 samples per mesh label is labelled here, with the same label -- or, where
    # sheets overlap, with the label of a later sheet that certainly passes through the cell and that the samples missed
    sampled = ref.sampled_all if which == "all" else ref.sampled[which]
    settled = np.ones(vo.SHAPE, dtype=bool)
    for must, may in bounds:
        settled &= must == may
    hit = (sampled != 0) & settled
    later = got > sampled
    print(f"cover {which}: sampled {int((sampled != 0).sum())} of {int((got != 0).sum())} cells, {int((hit & later).sum())} with a later label")
    assert (got[hit] >= sampled[hit]).all()
    for m, (must, _) in enumerate(bounds):
        assert must[hit & later & (got == m + 1)].all()
    if which == "all":                                                            # the real reference's own scatter of the same samples
        recorded = ref.golden["o3d_all"]
        assert np.array_equal(recorded, sampled)


def test_overlapping_sheets_highest_label_wins(fsg, device, ref):
    got = run_cover(fsg, device, ref.meshes, vo.SHAPE, vo.SPACING)
    both = ref.bounds[0][0] & ref.bounds[2][0] & ~ref.bounds[1][1]               # certainly sheets 0 and 2, certainly not 1
    assert both.sum() > 0 and (got[both] == 3).all()
    low = ref.bounds[0][0] & ref.bounds[1][0] & ~ref.bounds[2][1]
    assert low.sum() > 0 and (got[low] == 2).all()


# ---------------------------------------------------------------- small shapes where it can still go wrong
def _tri(*pts):
    return np.array(pts, dtype=np.float64) + 0.0137, np.array([[0, 1, 2]])


SMALL_SHAPE, SMALL_SPACING = (7, 9, 6), (1.25, 0.8, 1.0)
EMPTY = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))


def _small_cases():
    sheet_v, sheet_f = vo.sheet(4, 0.3, SMALL_SHAPE, SMALL_SPACING, n=11)
    ext = vo.extent(SMALL_SHAPE, SMALL_SPACING)
    a, b = np.array([2.1, 1.3, 0.7]), np.array([6.3, 5.9, 4.4])
    a2, b2 = np.array([5.5, 1.2, 4.1]), np.array([1.4, 6.0, 0.9])
    mid, d1, d2 = np.array(ext) / 2, np.array([1., 0.2, 0.1]), np.array([0.1, 1., 0.3])     # a plane through the centre
    return [
        ("one face", [_tri([2.2, 1.1, 0.6], [5.1, 6.3, 1.2], [3.3, 2.4, 4.9])], SMALL_SHAPE, SMALL_SPACING, 1.0),
        ("197 faces: no multiple of a wave or a workgroup", [(sheet_v, sheet_f[:197])], SMALL_SHAPE, SMALL_SPACING, 1.0),
        ("5 faces: a workgroup and a quarter", [(sheet_v, sheet_f[60:65])], SMALL_SHAPE, SMALL_SPACING, 1.0),
        ("a triangle larger than the volume", [_tri(mid - 40 * d1 - 30 * d2, mid + 50 * d1 - 20 * d2, mid - 10 * d1 + 60 * d2)],
         SMALL_SHAPE, SMALL_SPACING, 1.0),
        ("a mesh entirely outside", [_tri([ext[0] + 3, 1., 1.], [ext[0] + 5, 4., 1.], [ext[0] + 4, 2., 5.]),
                                     _tri([1., -9., 1.], [2., -4., 3.], [5., -6., 2.])], SMALL_SHAPE, SMALL_SPACING, 1.0),
        ("threshold below half the smallest spacing", [(sheet_v, sheet_f)], SMALL_SHAPE, SMALL_SPACING, 0.3),
        ("threshold 0", [(sheet_v, sheet_f)], SMALL_SHAPE, SMALL_SPACING, 0.0),
        ("faces without area", [(np.stack([a, b, a + 0.3 * (b - a)]), np.array([[0, 1, 2], [2, 0, 1]])),
                                (np.stack([b2, a2, a2]), np.array([[0, 1, 2]])),
                                (np.stack([a * 0.5, a * 0.5, a * 0.5, b]), np.array([[0, 1, 2], [0, 0, 0]]))], SMALL_SHAPE,
         SMALL_SPACING, 1.0),
        ("an empty mesh between two", [(sheet_v, sheet_f), EMPTY, _tri([2.2, 1.1, 0.6], [5.1, 6.3, 1.2], [3.3, 2.4, 4.9])],
         SMALL_SHAPE, SMALL_SPACING, 1.0),
        ("1 x 1 x N volume", [_tri([-0.4, -0.3, 3.2], [0.5, 0.4, 20.7], [0.3, -0.6, 11.1])], (1, 1, 37), (1.25, 0.8, 1.0), 1.0),
        ("N x 1 x 1 volume", [_tri([3.2, -0.3, -0.4], [30.7, 0.4, 0.5], [11.1, -0.6, 0.3])], (37, 1, 1), (1.25, 0.8, 1.0), 1.0),
    ]


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: c[0])
def test_small_shapes(fsg, device, case):
    name, meshes, shape, spacing, thr = case
    dist = vo.distances(meshes, shape, spacing)
    got = run_dist(fsg, device, meshes, shape, spacing, thr)
    labelled, excused, wrong, _ = vo.check_dist(got, dist, shape, thr)
    print(f"{name}: dist labelled {labelled} excused {excused} wrong {wrong}")
    assert wrong == 0
    cover = run_cover(fsg, device, meshes, shape, spacing)
    c_labelled, c_excused, c_wrong = vo.check_cover(cover, vo.cover_bounds(meshes, shape, spacing))
    print(f"{name}: cover labelled {c_labelled} excused {c_excused} wrong {c_wrong}")
    assert c_wrong == 0
    if name == "a mesh entirely outside":
        assert labelled == 0 and not got.any() and not cover.any()
    elif name == "threshold 0":
        assert c_labelled > 0
    else:
        assert labelled > 0 and c_labelled > 0
    if name == "an empty mesh between two":
        assert set(np.unique(got)) == {0, 1, 3} and set(np.unique(cover)) == {0, 1, 3}
    if name == "a triangle larger than the volume":
        assert labelled > 40                                                      # it does pass through


def test_all_meshes_empty_and_single_tensors(fsg, device):
    e = (torch.zeros(0, 3, device=device), torch.zeros(0, 3, dtype=torch.int64, device=device))
    assert not fsg.functional.mesh_labelmap_dist([e[0]], [e[1]], (3, 4, 5), (1., 1., 1.)).any()
    assert not fsg.functional.mesh_labelmap_cover([e[0], e[0]], [e[1], e[1]], (3, 4, 5), (1., 1., 1.)).any()
    v, f = _tri([1.2, 1.1, 0.6], [2.1, 3.3, 1.2], [1.3, 2.4, 3.9])
    one = fsg.functional.mesh_labelmap_dist(G(v, device, torch.float32), G(f, device), (3, 4, 5), (1., 1., 1.))
    assert torch.equal(one, fsg.functional.mesh_labelmap_dist([G(v, device, torch.float32)], [G(f, device)], (3, 4, 5), (1., 1., 1.)))
    assert one.any()


# ---------------------------------------------------------------- validation
def test_validation_raises_before_any_launch(fsg, device):
    v, f = _tri([1.2, 1.1, 0.6], [2.1, 3.3, 1.2], [1.3, 2.4, 3.9])
    good_v, good_f = G(v, device, torch.float32), G(f, device)
    for fn in (fsg.functional.mesh_labelmap_dist, fsg.functional.mesh_labelmap_cover):
        for bad in (float("nan"), float("inf"), -float("inf")):
            bv = good_v.clone()
            bv[1, 2] = bad
            with pytest.raises(ValueError, match="non-finite"):
                fn([good_v, bv], [good_f, good_f], (3, 4, 5), (1., 1., 1.))
        for bad in (3, -1):
            bf = good_f.clone()
            bf[0, 1] = bad
            with pytest.raises(ValueError, match="face indices"):
                fn([good_v, good_v], [good_f, bf], (3, 4, 5), (1., 1., 1.))
        with pytest.raises(ValueError, match="integer"):
            fn([good_v], [good_f.float()], (3, 4, 5), (1., 1., 1.))
        with pytest.raises(ValueError, match="as many"):
            fn([good_v, good_v], [good_f], (3, 4, 5), (1., 1., 1.))
        with pytest.raises(RuntimeError, match="spacing"):
            fn([good_v], [good_f], (3, 4, 5), (1., 0., 1.))
    with pytest.raises(ValueError, match="mask of shape"):
        fsg.functional.mesh_labelmap_dist([good_v], [good_f], (3, 4, 5), (1., 1., 1.), mask=torch.ones(3, 4, 4, device=device))
    with pytest.raises(RuntimeError, match="negative"):
        fsg.functional.mesh_labelmap_dist([good_v], [good_f], (3, 4, 5), (1., 1., 1.), dist_threshold=-1.0)


# ---------------------------------------------------------------- the reference's names and axis conventions
def test_wrappers_keep_the_reference_conventions(fsg, device, ref):
    from fissure_segmentation_amd.data_processing import surface_fitting as sf, surface_fitting_optimization as sfo
    spacing_xyz = vo.SPACING[::-1]
    pairs = [(G(v, device, torch.float32), G(f, device)) for v, f in ref.meshes]
    mask = G(ref.mask, device)
    # volume-order vertices, spacing given x, y, z and applied reversed
    got = sfo.mesh2labelmap_dist(pairs, vo.SHAPE, spacing_xyz, dist_threshold=1.5, mask=mask)
    assert got.dtype == torch.int64 and got.is_cuda
    assert vo.check_dist(N(got), ref.dist, vo.SHAPE, 1.5, ref.mask)[2] == 0
    assert np.array_equal(N(got), run_dist(fsg, device, ref.meshes, vo.SHAPE, vo.SPACING, 1.5, ref.mask))
    assert vo.check_dist(N(sfo.mesh2labelmap_dist(pairs, vo.SHAPE, spacing_xyz)), ref.dist, vo.SHAPE, 1.0)[2] == 0   # defaults
    direct = run_cover(fsg, device, ref.meshes, vo.SHAPE, vo.SPACING)
    sampling = sf.mesh2labelmap_sampling(pairs, vo.SHAPE, spacing_xyz, num_samples=123)
    assert vo.check_cover(N(sampling), ref.bounds)[2] == 0 and np.array_equal(N(sampling), direct)
    # x, y, z vertices: tensors, and duck meshes with numpy .vertices / .triangles
    flipped = [(v.flip(-1), f) for v, f in pairs]
    o3d = sf.o3d_mesh_to_labelmap(flipped, vo.SHAPE, spacing_xyz, n_samples=5)
    assert np.array_equal(N(o3d), direct)
    ducks = [SimpleNamespace(vertices=v[:, ::-1].astype(np.float32), triangles=f) for v, f in ref.meshes]
    ducks.insert(1, SimpleNamespace(vertices=np.zeros((0, 3)), triangles=np.zeros((0, 3), dtype=np.int64)))
    shifted = N(sf.o3d_mesh_to_labelmap(ducks, vo.SHAPE, spacing_xyz))
    assert np.array_equal(shifted, np.where(direct >= 2, direct + 1, direct))    # the empty mesh is skipped and keeps its label


def test_label_mesh_assd_is_mask_to_points_plus_the_point_to_mesh_distance(fsg, device, ref):
    from fissure_segmentation_amd import metrics
    from fissure_segmentation_amd.utils.general_utils import mask_to_points
    spacing_xyz = vo.SPACING[::-1]
    v, f = ref.meshes[0]
    mesh = (G(v[:, ::-1], device, torch.float32), G(f, device))                   # x, y, z like the points
    labelmap = fsg.functional.mesh_labelmap_dist([G(v, device, torch.float32)], [mesh[1]], vo.SHAPE, vo.SPACING, 1.0)
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    *got, points = metrics.label_mesh_assd(labelmap, mesh, spacing_xyz, n_samples=20000, generator=gen)
    want_points = mask_to_points(labelmap, spacing_xyz)
    assert torch.equal(points, want_points) and points.shape == (int((labelmap != 0).sum()), 3)
    gen.manual_seed(7)
    want = metrics.pseudo_symmetric_point_to_mesh_distance(want_points, mesh, 20000, gen)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == 4
    # the points are voxel centres within 1 mm of the mesh: the points -> mesh half of the mean is below the threshold
    d = metrics.point_surface_distance(points, *mesh)
    assert float(d.max()) <= 1.0 + 1e-4
