"""Marching cubes without a GPU: the generated case table (its properties recomputed here from the cube's geometry, not with the
generator's triangulation code), the numpy oracle the GPU tests compare against, the argument checks of the public entry
points and the signatures of the DPSR classes against the reference's."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import mc_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    from fissure_segmentation_amd import _mc_table
    return _mc_table


# ------------------------------------------------------------------ the cube, restated
CORNER = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
EDGE = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]     # ascending (a, b)


def _mid(e):
    a, b = CORNER[EDGE[e][0]], CORNER[EDGE[e][1]]
    return tuple((p + q) / 2 for p, q in zip(a, b))


def _on_one_face(e, f):
    pts = [CORNER[c] for c in EDGE[e] + EDGE[f]]
    return any(len({p[a] for p in pts}) == 1 for a in range(3))


def _expected_segments(case):
    """the directed face segments from geometry: on each face, seen from outside, every maximal run of inside corners met on a
    counter-clockwise walk is closed by one segment from the edge where the walk leaves the run to the edge where it entered"""
    segs = []
    for axis, side in itertools.product(range(3), (0, 1)):
        u, v = [a for a in range(3) if a != axis]
        outward = [0.0, 0.0, 0.0]
        outward[axis] = 1.0 if side else -1.0
        centre = [0.5, 0.5, 0.5]
        centre[axis] = float(side)
        ring = [c for c in range(8) if CORNER[c][axis] == side]
        # order by the angle round the outward normal: counter-clockwise as seen from outside
        e1 = [0.0, 0.0, 0.0]
        e1[u] = 1.0
        e2 = np.cross(outward, e1)
        ring.sort(key=lambda c: np.arctan2(np.dot(np.subtract(CORNER[c], centre), e2), np.dot(np.subtract(CORNER[c], centre), e1)))
        inside = [(case >> c) & 1 for c in ring]
        if sum(inside) in (0, 4):
            continue
        for i in range(4):
            if inside[i] and not inside[i - 1]:
                j = i
                while inside[(j + 1) % 4]:
                    j += 1
                left = tuple(sorted((ring[j % 4], ring[(j + 1) % 4])))
                entered = tuple(sorted((ring[i - 1], ring[i])))
                segs.append((EDGE.index(left), EDGE.index(entered)))
    return segs


def test_cube_layout():
    t = _table()
    assert [tuple(c) for c in t.CORNERS] == CORNER and [tuple(e) for e in t.EDGES] == EDGE and len(EDGE) == 12
    assert t.EDGE_AXIS == [(a ^ b).bit_length() - 1 for a, b in EDGE]


def test_boundary_of_every_case_is_its_face_segments():
    t = _table()
    for case in range(256):
        tris = t.TRIANGLES[case]
        directed = [(tri[k], tri[(k + 1) % 3]) for tri in tris for k in range(3)]
        assert len(set(directed)) == len(directed), f"case {case}: a directed edge twice"
        boundary = sorted(d for d in directed if (d[1], d[0]) not in directed)
        # triangles are wound against the loops (normals toward increasing values), so the boundary is the reversed segments
        assert boundary == sorted((b, a) for a, b in _expected_segments(case)), f"case {case}"
        interior = [d for d in directed if (d[1], d[0]) in directed]
        assert not any(_on_one_face(a, b) for a, b in interior), f"case {case}: a diagonal inside a cube face"


def test_table_sizes_and_complements():
    t = _table()
    counts = [len(x) for x in t.TRIANGLES]
    assert max(counts) == 5 and sum(counts) == 820 and counts[0] == 0 and counts[255] == 0
    assert all(c > 0 for c in counts[1:255])
    for case in range(256):
        used = {e for tri in t.TRIANGLES[case] for e in tri}
        crossing = {e for e, (a, b) in enumerate(EDGE) if ((case >> a) ^ (case >> b)) & 1}
        assert used == crossing
        assert used == {e for tri in t.TRIANGLES[255 - case] for e in tri}


def test_triangles_face_the_increasing_values():
    t = _table()
    for case in range(1, 255):
        inside = np.array([CORNER[c] for c in range(8) if (case >> c) & 1], float)
        outside = np.array([CORNER[c] for c in range(8) if not (case >> c) & 1], float)
        n = np.zeros(3)
        for tri in t.TRIANGLES[case]:
            p = np.array([_mid(e) for e in tri])
            n += np.cross(p[1] - p[0], p[2] - p[0])
        if len(t.loops(case)) == 1:      # one sheet: its summed normal points from the inside corners to the outside ones
            assert np.dot(n, outside.mean(0) - inside.mean(0)) > 0, case


def test_committed_header_is_the_generators_output():
    path = os.path.join(ROOT, "fissure-segmentation_amd", "csrc", "mc_table.h")
    assert open(path).read() == _table().header(), "run tools/gen_mc_table.py"


# ------------------------------------------------------------------ the oracle
def _padded(inner):
    out = np.ones(tuple(s + 2 for s in inner.shape), np.float32)
    out[1:-1, 1:-1, 1:-1] = inner
    return out


@pytest.mark.parametrize("seed", range(6))
def test_oracle_is_closed_and_oriented(seed):
    field = _padded(np.random.default_rng(seed).standard_normal((9, 10, 11)).astype(np.float32))
    v, f, n = mo.marching_cubes_item(field, 0.0, False)
    assert len(f) > 0 and mo.directed_edge_defect(f) == (0, 0)
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    assert mo.signed_volume(v, f) > 0          # the region below the level is enclosed with outward normals


def test_oracle_sphere():
    z, y, x = np.mgrid[:16, :16, :16]
    field = (np.sqrt((x - 7.5) ** 2 + (y - 7.5) ** 2 + (z - 7.5) ** 2) - 5).astype(np.float32)
    v, f, n = mo.marching_cubes_item(field, 0.0, False)
    assert mo.euler_characteristic(f) == 2
    assert ((v - 7.5) * n).sum(1).min() > 0
    vol = mo.signed_volume(v, f)
    assert 0.95 * 523.6 < vol < 523.6          # inscribed in the sphere of radius 5
    vl, fl, _ = mo.marching_cubes_item(field, 0.0, True)
    assert np.array_equal(f, fl) and np.allclose(vl, 2 * v / 15 - 1, atol=1e-12)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_oracle_vertices_lie_on_their_edges_at_the_level(dtype):
    field = np.random.default_rng(3).standard_normal((6, 7, 8)).astype(np.float32)
    iso = 0.2
    v, f, n = mo.marching_cubes_item(field, iso, False, dtype=dtype)
    assert v.dtype == dtype and n.dtype == dtype
    frac = v - np.floor(v)
    assert ((frac > 0).sum(1) <= 1).all()                                  # on a grid edge: at most one non-integer coordinate
    lo = np.floor(v).astype(int)
    hi = np.minimum(lo + (frac > 0), np.array(field.shape[::-1]) - 1)
    fa, fb = field[lo[:, 2], lo[:, 1], lo[:, 0]].astype(np.float64), field[hi[:, 2], hi[:, 1], hi[:, 0]].astype(np.float64)
    t = frac.max(1)
    value = fa + t * (fb - fa)
    assert np.abs(value - np.float32(iso)).max() < (1e-12 if dtype == np.float64 else 1e-5)
    assert ((fa < np.float32(iso)) != (fb < np.float32(iso)))[t > 0].all()


def test_oracle_mask_leaves_no_unreferenced_vertex():
    field = np.random.default_rng(4).standard_normal((7, 8, 9)).astype(np.float32)
    mask = np.ones(field.shape, np.uint8)
    mask[:, :, 5:] = 0
    v, f, n = mo.marching_cubes_item(field, 0.0, True, mask=mask)
    full = mo.marching_cubes_item(field, 0.0, True)
    assert 0 < len(f) < len(full[1]) and np.array_equal(np.unique(f), np.arange(len(v)))
    assert v[:, 0].max() <= 2 * 4 / 8 - 1 + 1e-12                          # nothing past the last node in the mask


# ------------------------------------------------------------------ argument checks
def test_argument_checks_and_gpu_only():
    from fissure_segmentation_amd import functional as F
    ok = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="(?i)GPU only"):
        F.marching_cubes(ok)
    with pytest.raises(RuntimeError, match="(?i)GPU only"):
        F.marching_cubes_labels(torch.zeros(4, 4, 4, dtype=torch.int64), 1, 2)
    with pytest.raises(TypeError):
        F.marching_cubes(ok.long())
    for bad in (torch.zeros(4, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 4, 4, 1), torch.zeros(0, 4, 4, 4)):
        with pytest.raises(ValueError):
            F.marching_cubes(bad)
    with pytest.raises(ValueError, match="mask"):
        F.marching_cubes(ok, mask=torch.ones(1, 4, 4, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        F.marching_cubes(ok, mask=torch.ones(1, 4, 4, 4))
    with pytest.raises(ValueError, match="isolevel"):
        F.marching_cubes(ok, isolevel=float("nan"))
    with pytest.raises(ValueError):
        F.marching_cubes_labels(torch.zeros(4, 4, 4), 1, 2)
    with pytest.raises(ValueError):
        F.marching_cubes_labels(torch.zeros(4, 4, 4, dtype=torch.int64), 1, 0)
    with pytest.raises(ValueError, match="spacing"):
        F.marching_cubes_labels(torch.zeros(4, 4, 4, dtype=torch.int64), 1, 2, spacing=(1, 0, 1))
    with pytest.raises(ValueError, match="spacing"):
        F.marching_cubes_labels(torch.zeros(4, 4, 4, dtype=torch.int64), 1, 2, spacing=(1, 1))


def test_library_checks_before_any_launch():
    from fissure_segmentation_amd import _lib
    assert _lib.lib.fsg_mc_workspace_bytes(1, 2, 2, 2) > 0 and _lib.lib.fsg_mc_workspace_bytes(1, 1, 2, 2) == 0
    assert _lib.lib.fsg_mc_workspace_bytes(2, 1024, 1024, 1024) == 0
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("fsg_mc_count_f32", 1, None, 0, 1, 1, 4, 4, 0.0, 1, 1, 1 << 20, 1, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_mc_count_f32", None, None, 0, 1, 4, 4, 4, 0.0, 1, 1, 1 << 20, 1, None)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("fsg_mc_count_f32", 8, None, 0, 1, 4, 4, 4, 0.0, 1, 8, 16, 8, None)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("fsg_mc_emit_labels_i32", 8, 1, 1, 4, 4, 4, 0, 1.0, 1.0, 1.0, 4, 1 << 20, 8, 1, 1, 8, 8, 8, None)
    with pytest.raises(RuntimeError, match="mask_item_stride"):
        _lib.call("fsg_mc_count_labels_i32", 8, 8, 5, 1, 2, 4, 4, 4, 8, 1 << 20, 8, None)


def test_meshes_carry_normals():
    from fissure_segmentation_amd.mesh import Meshes, join_meshes_as_batch
    v = [torch.rand(4, 3), torch.rand(5, 3)]
    f = [torch.tensor([[0, 1, 2], [0, 2, 3]]), torch.tensor([[0, 1, 2]])]
    n = [torch.rand(4, 3), torch.rand(5, 3)]
    m = Meshes(v, f, verts_normals=n)
    assert torch.equal(m.verts_normals_packed(), torch.cat(n)) and m.verts_normals_padded().shape == (2, 5, 3)
    assert torch.equal(m.verts_normals_padded()[0, :4], n[0]) and not m.verts_normals_padded()[0, 4:].any()
    assert m.faces_padded().tolist() == [[[0, 1, 2], [0, 2, 3]], [[0, 1, 2], [-1, -1, -1]]]
    assert torch.equal(m[1].verts_normals_list()[0], n[1])
    assert torch.equal(join_meshes_as_batch([m[0], m[1]]).verts_normals_packed(), torch.cat(n))
    p = Meshes(torch.rand(2, 4, 3), f[0], torch.rand(2, 4, 3))
    assert p.verts_normals_packed().shape == (8, 3) and p.faces_padded().shape == (2, 2, 3)
    plain = Meshes(v, f)
    for call in (plain.verts_normals_list, plain.verts_normals_packed, plain.verts_normals_padded):
        with pytest.raises(NotImplementedError, match="carried"):
            call()
    with pytest.raises(ValueError, match="verts_normals"):
        Meshes(v, f, [n[0]])
    with pytest.raises(ValueError, match="verts_normals"):
        Meshes(torch.rand(2, 4, 3), f[0], torch.rand(2, 5, 3))


# ------------------------------------------------------------------ signatures against the reference's
def _ref_signature(path, cls, fn):
    """the parameter names (and defaults, as source text) of `cls.fn` in a source file, read with ast"""
    import ast
    tree = ast.parse(open(path).read())
    node = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
    f = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == fn)
    names = [a.arg for a in f.args.args]
    defaults = [ast.unparse(d) for d in f.args.defaults]
    return names, defaults


# recorded from the reference (models/seg_logits_to_mesh.py:16-18, losses/dpsr_loss.py:16, :28, models/dpsr_utils.py:52, :67, :78)
RECORDED = {
    ("models/seg_logits_to_mesh.py", "DPSRNet2", "__init__"): (
        ["self", "seg_net_class", "k", "in_features", "num_classes", "spatial_transformer", "dynamic", "image_feat_module",
         "normals_smoothing_sigma", "dpsr_res", "dpsr_sigma", "dpsr_scale", "dpsr_shift"],
        ["False", "True", "False", "10", "(128, 128, 128)", "10", "True", "True"]),
    ("models/seg_logits_to_mesh.py", "DPSRNet2", "forward"): (["self", "x"], []),
    ("models/seg_logits_to_mesh.py", "DPSRNet2", "predict_full_pointcloud"): (["self", "pc", "sample_points", "n_runs_min"], ["1024", "50"]),
    ("losses/dpsr_loss.py", "DPSRLoss", "__init__"): (
        ["self", "class_weights", "w_seg", "w_mesh", "epoch_start_mesh_loss"],
        ["DEFAULT_W_SEG", "DEFAULT_W_CHAMFER", "DEFAULT_EPOCH_START_CHAMFER"]),
    ("losses/dpsr_loss.py", "DPSRLoss", "forward"): (["self", "prediction", "target", "current_epoch_fraction"], ["None"]),
    ("models/dpsr_utils.py", "DifferentiableMarchingCubes", "forward"): (["psr_grid"], []),
    ("models/dpsr_utils.py", "DifferentiableMarchingCubes", "setup_context"): (["ctx", "inputs", "output"], []),
    ("models/dpsr_utils.py", "DifferentiableMarchingCubes", "backward"): (["ctx", "dL_dVertex", "dL_dFace", "dL_dNormals"], []),
}


@pytest.mark.parametrize("key", sorted(RECORDED))
def test_signatures_are_the_references(key):
    rel, cls, fn = key
    ours = os.path.join(ROOT, "fissure-segmentation_amd", rel)
    assert _ref_signature(ours, cls, fn) == RECORDED[key]


def test_dpsr_classes():
    from fissure_segmentation_amd.losses.dpsr_loss import DPSRLoss
    from fissure_segmentation_amd.losses.mesh_loss import RegularizedMeshLossHIP
    from fissure_segmentation_amd.models.dpsr_utils import DifferentiableMarchingCubes
    from fissure_segmentation_amd.models.seg_logits_to_mesh import DPSRNet2, SoftMesh
    net = DPSRNet2("DGCNN", k=4, in_features=3, num_classes=3, dpsr_res=(8, 8, 8))
    assert isinstance(net.seg2mesh, SoftMesh) and net.res == (8, 8, 8) and net.config["num_classes"] == 3
    keys = set(net.state_dict())
    assert "seg2mesh.dpsr.G" in keys and all(k.startswith(("seg_net.", "seg2mesh.")) for k in keys)
    with pytest.raises(NotImplementedError, match="never defines"):
        net.predict_full_pointcloud(torch.zeros(1, 3, 8))
    loss = DPSRLoss(None)
    assert (loss.w_seg, loss.w_mesh, loss.epoch_start_mesh) == (0.5, 0.5, 0.1)
    assert isinstance(loss.chamfer_loss, RegularizedMeshLossHIP)
    c = loss.chamfer_loss
    assert (c.w_chamfer, c.w_edge_length, c.w_normal_consistency, c.w_laplacian) == (1, 0, 0, 0)
    assert issubclass(DifferentiableMarchingCubes, torch.autograd.Function)
    assert inspect.signature(SoftMesh.meshes).parameters.keys() == inspect.signature(SoftMesh.forward).parameters.keys()
    with pytest.raises(RuntimeError, match="(?i)GPU only"):
        DifferentiableMarchingCubes.apply(torch.zeros(1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="(?i)GPU only"):
        from fissure_segmentation_amd.data_processing.find_lobes import compute_surface_mesh_marching_cubes
        compute_surface_mesh_marching_cubes(torch.zeros(4, 4, 4, dtype=torch.int64))


def test_reference_import_names_and_untouched_registry():
    """the DPSR modules answer to the reference's import names; get_loss_fn('dpsr') keeps refusing (the class is opt-in)"""
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from losses.access_losses import get_loss_fn
        from losses.dpsr_loss import DPSRLoss
        from models.dpsr_utils import DifferentiableMarchingCubes  # noqa: F401
        from models.seg_logits_to_mesh import DPSRNet2, SoftMesh  # noqa: F401
        assert "fissure" in DPSRLoss.__module__ and "fissure" in DPSRNet2.__module__
        with pytest.raises(NotImplementedError, match="outside the MI355X hot path"):
            get_loss_fn("dpsr")
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
