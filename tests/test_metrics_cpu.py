"""CPU tests of the metrics feature: the fp64 point-triangle oracle (tests/metrics_oracle.py) against closed forms -- it is
what the kernel is held to on the GPU, and open3d, the reference's implementation, is not available to pin it --, degenerate
faces, the summary functions against the real reference's recorded outputs, and the host-side contract of
fissure_segmentation_amd.metrics (imports without a GPU, refuses CPU tensors)."""
import math

import numpy as np
import pytest
import torch

import metrics_oracle as mo
from golden_util import load

D = torch.float64
# the one triangle probed region by region: right angle at a
TRI_V = [[0., 0., 0.], [2., 0., 0.], [0., 1., 0.]]
TRI_F = [[0, 1, 2]]
SEVEN_REGIONS = [   # (region, query, closed-form distance)
    ("interior", [0.5, 0.25, 0.7], 0.7),
    ("vertex a", [-1., -2., 0.5], math.sqrt(1 + 4 + 0.25)),
    ("vertex b", [3., -0.5, 0.], math.sqrt(1 + 0.25)),
    ("vertex c", [-0.5, 3., 1.], math.sqrt(0.25 + 4 + 1)),
    ("edge ab", [1., -2., 0.], 2.0),
    ("edge ac", [-3., 0.5, 4.], 5.0),
    ("edge bc", [2., 1., 0.], 2 / math.sqrt(5)),          # line x + 2y = 2: (2 + 2 - 2) / sqrt(5), foot (1.6, 0.2) on the edge
]


def closed_form_cases():
    """(name, pts (P,3), verts (V,3), faces (F,3), expected distances (P,)) -- shared with tests/test_metrics_gpu.py"""
    from fissure_segmentation_amd.shapes.shape_constructor import get_plane_mesh
    xy, faces = get_plane_mesh(n=81)                                      # 9 x 9 vertices over [-1, 1]^2, z = 0
    verts = torch.cat([xy, torch.zeros(len(xy), 1)], 1).numpy().astype(np.float64)
    faces = faces.numpy()
    rng = np.random.default_rng(5)
    above = np.concatenate([rng.uniform(-1, 1, (64, 2)), rng.uniform(-2, 2, (64, 1))], 1)
    beyond = np.array([[1.5, 0.3, 0.4], [-1.25, -0.9, -1.0], [0.1, 2.0, 0.0], [0.2, -1.5, 2.0]])       # beyond one edge of the square
    beyond_d = [math.hypot(0.5, 0.4), math.hypot(0.25, 1.0), 1.0, math.hypot(0.5, 2.0)]
    corner = np.array([[1.5, 1.5, 0.], [-2., 1.25, 1.], [-1.5, -3., -0.5], [4., -1.5, 0.25]])         # beyond a corner
    corner_d = [math.sqrt(0.5), math.sqrt(1 + 0.0625 + 1), math.sqrt(0.25 + 4 + 0.25), math.sqrt(9 + 0.25 + 0.0625)]
    w = rng.dirichlet((1, 1, 1), len(faces))
    on_mesh = np.concatenate([(verts[faces] * w[:, :, None]).sum(1), verts, verts[faces][:, :2].mean(1)])   # faces, vertices, edges
    cases = [("above the plane", above, verts, faces, np.abs(above[:, 2])), ("beyond an edge", beyond, verts, faces, beyond_d),
             ("beyond a corner", corner, verts, faces, corner_d), ("on the mesh", on_mesh, verts, faces, np.zeros(len(on_mesh)))]
    for name, q, d in SEVEN_REGIONS:
        cases.append(("single triangle, " + name, np.array([q]), np.array(TRI_V), np.array(TRI_F), [d]))
    return [(n, np.asarray(p, dtype=np.float64), v, f, np.asarray(d, dtype=np.float64)) for n, p, v, f, d in cases]


def degenerate_cases():
    """(name, pts, verts, faces, expected): collinear faces are their longest edge, collapsed ones their point"""
    rng = np.random.default_rng(6)
    q = rng.uniform(-2, 2, (50, 3))
    a, b = np.array([-0.5, 0.25, 0.]), np.array([1.5, 1.25, 1.0])
    mid = a + 0.3 * (b - a)                                               # between a and b: the face (a, b, mid) has no area
    t = np.clip(((q - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
    seg = np.linalg.norm(q - (a + t[:, None] * (b - a)), axis=1)
    pt = np.linalg.norm(q - a, axis=1)
    return [("collinear, longest edge first", q, np.stack([a, b, mid]), np.array([[0, 1, 2]]), seg),
            ("collinear, longest edge last", q, np.stack([mid, a, b]), np.array([[0, 1, 2]]), seg),
            ("collinear, longest edge ac", q, np.stack([a, mid, b]), np.array([[0, 1, 2]]), seg),
            ("two vertices equal", q, np.stack([a, a, b]), np.array([[0, 1, 2]]), seg),
            ("all vertices equal", q, np.stack([a, a, a]), np.array([[0, 1, 2], [2, 1, 0]]), pt),
            ("same index three times", q, np.stack([b, a]), np.array([[1, 1, 1]]), pt)]


@pytest.mark.parametrize("case", closed_form_cases(), ids=lambda c: c[0])
def test_oracle_fp64_closed_forms(case):
    _, pts, verts, faces, want = case
    d2, face = mo.point_mesh_dist2(pts, verts, faces)
    assert d2.dtype == D and face.shape == (len(pts),)
    np.testing.assert_allclose(d2.sqrt().numpy(), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", degenerate_cases(), ids=lambda c: c[0])
def test_oracle_degenerate_faces_are_segments_or_points(case):
    _, pts, verts, faces, want = case
    d = mo.point_mesh_dist2(pts, verts, faces)[0].sqrt().numpy()
    assert np.isfinite(d).all()
    np.testing.assert_allclose(d, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", closed_form_cases() + degenerate_cases(), ids=lambda c: c[0])
def test_kernel_order_fp32_restatement_agrees(case):
    """the fp32 restatement in the kernel's operation order computes the same quantity: within fp32 rounding of the closed form
    (coordinates up to 4: a few 1e-7 relative to them) -- including the faces without area"""
    _, pts, verts, faces, want = case
    d = mo.kernel_order_dist2(pts, verts, faces).sqrt().numpy()
    assert d.dtype == np.float32 and np.isfinite(d).all()
    np.testing.assert_allclose(d, want, rtol=0, atol=5e-6)


def test_oracle_face_index_is_lowest_on_ties():
    """a query above a shared edge is equally far from both faces"""
    verts = np.array([[0., 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    faces = np.array([[1, 2, 3], [0, 1, 2], [0, 1, 2]])
    d2, face = mo.point_mesh_dist2(np.array([[0.5, 0.5, 1.0], [0.2, 0.2, 0.5]]), verts, faces)
    assert face.tolist() == [0, 1] and np.allclose(d2.numpy(), [1.0, 0.25])


def test_oracle_summaries_match_the_reference():
    g = load("metrics_torch")
    d1, d2 = mo.summary_inputs()
    assert int(g["summary_seed"]) == mo.SUMMARY_SEED and int(g["label_seed"]) == mo.LABEL_SEED
    np.testing.assert_allclose([float(x) for x in mo.symmetric_point_distances(d1, d2)], g["symmetric"], rtol=2e-6)
    pred, targ = mo.label_inputs()
    np.testing.assert_allclose(mo.batch_dice(pred, targ, mo.LABEL_N), g["dice"], rtol=1e-6)
    np.testing.assert_allclose(mo.binary_recall(pred, targ), g["recall"], rtol=1e-6)
    np.testing.assert_allclose(mo.binary_precision(pred, targ), g["precision"], rtol=1e-6)


def test_package_torch_functions_match_the_reference():
    """the functions of the package that are plain torch run on the CPU and reproduce the real reference's outputs"""
    from fissure_segmentation_amd import metrics
    g = load("metrics_torch")
    d1, d2 = (torch.from_numpy(a) for a in mo.summary_inputs())
    got = metrics._symmetric_point_distances(d1, d2)
    assert all(t.dim() == 0 for t in got)
    np.testing.assert_allclose([float(x) for x in got], g["symmetric"], rtol=2e-6)
    pred, targ = (torch.from_numpy(a) for a in mo.label_inputs())
    dice = metrics.batch_dice(pred, targ, mo.LABEL_N)
    assert dice.device.type == "cpu" and dice.shape == (mo.LABEL_N,)
    np.testing.assert_allclose(dice.numpy(), g["dice"], rtol=1e-6)
    np.testing.assert_allclose(metrics.binary_recall(pred, targ).numpy(), g["recall"], rtol=1e-6)
    np.testing.assert_allclose(metrics.binary_precision(pred, targ).numpy(), g["precision"], rtol=1e-6)


def test_metrics_import_and_refuse_cpu_tensors():
    import fissure_segmentation_amd as fsg
    from fissure_segmentation_amd import metrics
    assert not hasattr(metrics, "label_label_assd")
    pts, verts, faces = torch.zeros(5, 3), torch.tensor(TRI_V), torch.tensor(TRI_F)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.point_surface_distance(pts, verts, faces)
    with pytest.raises(RuntimeError, match="GPU"):
        fsg.functional.point_mesh_distance(pts[None], verts[None], faces)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.batch_assd(verts[None], faces[None], verts[None], faces[None])
    empty = (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.long))
    out = metrics.assd(empty, (verts, faces))                             # decided on the host, like metrics.py:35-36
    assert len(out) == 4 and all(torch.isnan(t) for t in out)


def test_alias_and_quantile_cap():
    import sys
    import fissure_segmentation_amd as fsg
    from fissure_segmentation_amd import metrics
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        import metrics as aliased
        # (not `is metrics`: tests that restore sys.modules make the package re-import its submodules)
        assert aliased.__name__ == "fissure_segmentation_amd.metrics" and aliased.__file__ == metrics.__file__
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
    with pytest.raises(AssertionError, match="16000000"):
        metrics._quantile95(torch.zeros(1).expand(metrics.QUANTILE_MAX_ELEMENTS + 1))


def test_bad_arguments_are_reported():
    from fissure_segmentation_amd import _lib
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_point_mesh_dist_f32", None, None, None, 1, 8, 3, 1, 1, None, None, None, None)
