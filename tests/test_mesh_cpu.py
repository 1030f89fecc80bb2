"""CPU tests of the mesh pieces (fissure_segmentation_amd/mesh.py, csrc/mesh.hip, losses/mesh_loss.py:RegularizedMeshLossHIP):
the C ABI's declarations and host-side argument checks, the host-built topology against the brute-force oracle
(tests/mesh_oracle.py) and against counts worked out by hand, the `Meshes` container, and the opt-in switches."""
import inspect
import re

import pytest
import torch

import mesh_oracle
from conftest import ROOT

NEW_SYMBOLS = ("fsg_mesh_reg_workspace_bytes", "fsg_mesh_reg_f32", "fsg_mesh_sample_workspace_bytes", "fsg_mesh_sample_f32",
               "fsg_mesh_sample_bwd_f32")


def _plane(n):
    from fissure_segmentation_amd.shapes.shape_constructor import get_plane_mesh
    p, f = get_plane_mesh(n)
    return torch.cat([p, torch.zeros(p.shape[0], 1)], 1), f


TET = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
FAN = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 1, 4]])


def test_symbols_declared_bound_and_exported():
    import os
    from fissure_segmentation_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    declared = set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "mesh.hip" in open(os.path.join(ROOT, "fissure-segmentation_amd", "csrc", "Makefile")).read()
    assert _lib.lib.fsg_mesh_reg_workspace_bytes(32, 2025) == 32 * 8 * 3 * 8      # 8 chunks of 256 vertices, 3 fp64 sums
    assert _lib.lib.fsg_mesh_reg_workspace_bytes(0, 5) == 0
    assert _lib.lib.fsg_mesh_sample_workspace_bytes(3, 100) == 3 * 100 * 8


def test_bad_arguments_are_reported_before_launch():
    """validation is on the host and comes first, so it is testable without a GPU (1 / 8 stand for non-NULL pointers)"""
    from fissure_segmentation_amd import _lib
    ok = [8] * 5
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_mesh_reg_f32", None, 4, 8, 1, 4, *ok, 8, 8, None, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_mesh_reg_f32", 8, 4, 8, 1, 4, 8, 8, None, 8, 8, 8, 8, None, 8, 1 << 20, None)
    for N, max_v, total in ((0, 4, 4), (70000, 4, 4), (1, 0, 4), (1, 5, 4), (1, 4, 1 << 31)):
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_mesh_reg_f32", 8, total, 8, N, max_v, *ok, 8, 8, None, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("fsg_mesh_reg_f32", 8, 4, 8, 1, 4, *ok, 8, 8, None, 4, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace of 23 bytes"):
        _lib.call("fsg_mesh_reg_f32", 8, 4, 8, 1, 4, *ok, 8, 8, None, 8, 23, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_mesh_sample_f32", 8, 8, 8, 1, 4, None, 16, 8, 8, 8, 8, 1 << 20, None)
    for N, max_f, n in ((0, 4, 16), (1, 0, 16), (1, 4, 0), (65536, 4, 16), (65535, 4, 1 << 20)):
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_mesh_sample_f32", 8, 8, 8, N, max_f, 8, n, 8, 8, 8, 8, 1 << 40, None)
    with pytest.raises(RuntimeError, match="workspace of 31 bytes"):
        _lib.call("fsg_mesh_sample_f32", 8, 8, 8, 1, 4, 8, 16, 8, 8, 8, 8, 31, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_mesh_sample_bwd_f32", 8, 8, 8, 8, 8, 1, 4, 16, None, None)
    for N, max_v, n in ((0, 4, 16), (1, 0, 16), (1, 4, 0)):
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_mesh_sample_bwd_f32", 8, 8, 8, 8, 8, N, max_v, n, 8, None)


def _same_topology(t, o, V):
    """the host-built topology against the brute-force one, list by list"""
    assert torch.equal(t["edges"], o["edges"]) and torch.equal(t["pairs"], o["pairs"]) and torch.equal(t["deg"], o["deg"])
    for i in range(V):
        mine = t["nbr"][t["nbr_off"][i]:t["nbr_off"][i + 1]].tolist()
        assert mine == sorted(o["dst"][o["src"] == i].tolist())
        codes = t["inc"][t["inc_off"][i]:t["inc_off"][i + 1]].tolist()
        assert codes == sorted(codes)
        assert codes == [4 * p + r for p in range(o["pairs"].shape[0]) for r in range(4) if int(o["pairs"][p, r]) == i]


@pytest.mark.parametrize("n,V,F,E,P", [(25, 25, 32, 56, 40), (2048, 2025, 3872, 5896, 5720)])
def test_plane_topology_counts(n, V, F, E, P):
    from fissure_segmentation_amd.mesh import build_topology
    v, f = _plane(n)
    assert (v.shape[0], f.shape[0]) == (V, F)
    t, o = build_topology(f, V), mesh_oracle.brute_topology(f, V)
    assert (t["E"], t["P"], o["edges"].shape[0], o["pairs"].shape[0]) == (E, P, E, P)
    if n == 25:
        _same_topology(t, o, V)
    else:
        assert torch.equal(t["edges"], o["edges"]) and torch.equal(t["pairs"], o["pairs"]) and torch.equal(t["deg"], o["deg"])


def test_flat_grid_normal_term_is_exactly_zero_on_the_oracle():
    """get_plane_mesh winds its two triangles per cell oppositely: per-face normals alternate in sign, the pair form does not care"""
    v, f = _plane(25)
    tri = v.double()[f]
    nz = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])[:, 2]
    assert bool((nz[0::2] * nz[1::2] < 0).all()) and bool((nz[0::2] * nz[0] > 0).all())        # the sign alternates
    for dtype in (torch.float64, torch.float32):
        mean, grads, _ = mesh_oracle.batch_terms([v], [mesh_oracle.brute_topology(f, 25)], dtype)
        assert float(mean[1]) == 0.0 and float(grads[1][0].abs().max()) == 0.0


def test_small_topologies():
    from fissure_segmentation_amd.mesh import build_topology
    t = build_topology(TET, 4)
    assert (t["E"], t["P"]) == (6, 6) and t["deg"].tolist() == [3, 3, 3, 3]
    _same_topology(t, mesh_oracle.brute_topology(TET, 4), 4)
    t = build_topology(FAN, 5)                                        # three faces on the edge (0, 1): three pairs
    assert (t["E"], t["P"]) == (7, 3)
    assert t["pairs"].tolist() == [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 3, 4]]
    _same_topology(t, mesh_oracle.brute_topology(FAN, 5), 5)
    t = build_topology(TET, 5)                                        # vertex 4 is in no face
    assert t["deg"].tolist() == [3, 3, 3, 3, 0] and int(t["nbr_off"][5] - t["nbr_off"][4]) == 0
    assert int(t["inc_off"][5] - t["inc_off"][4]) == 0
    _same_topology(t, mesh_oracle.brute_topology(TET, 5), 5)
    t = build_topology(torch.zeros(0, 3, dtype=torch.int64), 3)
    assert (t["E"], t["P"]) == (0, 0) and t["deg"].tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="span"):
        build_topology(TET, 3)
    with pytest.raises(ValueError, match="twice"):
        build_topology(torch.tensor([[0, 0, 1]]), 2)
    with pytest.raises(ValueError, match="integer"):
        build_topology(torch.zeros(2, 3), 4)


def test_meshes_round_trips():
    from fissure_segmentation_amd.mesh import Meshes, join_meshes_as_batch
    g = torch.Generator().manual_seed(0)
    vp, fp = _plane(25)
    verts = [torch.rand(4, 3, generator=g), torch.rand(5, 3, generator=g), vp]
    faces = [TET, FAN, fp]
    m = Meshes(verts, faces)
    assert len(m) == 3 and m.device == torch.device("cpu")
    assert m.num_verts_per_mesh().tolist() == [4, 5, 25] and m.num_faces_per_mesh().tolist() == [4, 3, 32]
    assert torch.equal(m.verts_packed(), torch.cat(verts)) and m.verts_packed().shape == (34, 3)
    packed = m.faces_packed()
    assert packed.shape == (39, 3) and torch.equal(packed[4:7], FAN + 4) and torch.equal(packed[7:], fp + 9)
    pad = m.verts_padded()
    assert pad.shape == (3, 25, 3) and torch.equal(pad[0, :4], verts[0]) and float(pad[0, 4:].abs().max()) == 0
    assert all(torch.equal(a, b) for a, b in zip(m.verts_list(), verts))
    assert all(torch.equal(a, b) for a, b in zip(m.faces_list(), faces))
    # indexing
    one = m[1]
    assert isinstance(one, Meshes) and len(one) == 1 and torch.equal(one.verts_list()[0], verts[1])
    assert m[1:].num_verts_per_mesh().tolist() == [5, 25] and m[[2, 0]].num_faces_per_mesh().tolist() == [32, 4]
    assert m[torch.tensor([True, False, True])].num_verts_per_mesh().tolist() == [4, 25]
    # tensor form, shared and per-mesh faces
    vb = torch.rand(2, 25, 3, generator=g)
    for fb in (fp, fp[None].expand(2, -1, -1)):
        s = Meshes(vb, fb)
        assert len(s) == 2 and torch.equal(s.verts_padded(), vb) and torch.equal(s.verts_packed(), vb.reshape(-1, 3))
        assert torch.equal(s.faces_packed(), torch.cat([fp, fp + 25])) and torch.equal(s.faces_list()[1], fp)
        assert torch.equal(Meshes(s.verts_list(), s.faces_list()).verts_padded(), vb)
    # joining
    j = join_meshes_as_batch([m, s, one])
    assert len(j) == 6 and j.num_verts_per_mesh().tolist() == [4, 5, 25, 25, 25, 5]
    assert torch.equal(j.verts_list()[4], vb[1]) and torch.equal(j.faces_list()[5], FAN)
    assert m.to("cpu") is m
    for bad in ((torch.rand(2, 5), fp), (vb, torch.zeros(3, 4, 3, dtype=torch.int64)), (vb, fp.float()),
                ([verts[0]], [TET, FAN])):
        with pytest.raises(ValueError):
            Meshes(*bad)


def test_cpu_tensors_are_refused():
    from fissure_segmentation_amd.losses.mesh_loss import RegularizedMeshLossHIP
    from fissure_segmentation_amd.mesh import (Meshes, mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency,
                                               mesh_regularizers, sample_points_from_meshes)
    v, f = _plane(25)
    m = Meshes(v[None], f)
    for fn in (mesh_regularizers, mesh_edge_loss, mesh_normal_consistency, mesh_laplacian_smoothing,
               lambda x: sample_points_from_meshes(x, 8), lambda x: x.sample_points(8), lambda x: RegularizedMeshLossHIP()(x, x)):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(m)
    with pytest.raises(NotImplementedError):
        mesh_laplacian_smoothing(m, method="cot")
    with pytest.raises(NotImplementedError):
        mesh_edge_loss(m, target_length=0.3)
    with pytest.raises(TypeError):
        mesh_regularizers(v)
    with pytest.raises(TypeError, match="return_meshes"):
        RegularizedMeshLossHIP()(v[None], v[None])


def test_new_names_leave_the_old_ones_alone():
    """the capability is opt-in: the loss has the reference's constructor plus `generator`, the registry name stays closed,
    `return_meshes` is a class attribute that `config` (and so a checkpoint) does not know"""
    from fissure_segmentation_amd.losses.access_losses import get_loss_fn
    from fissure_segmentation_amd.losses.mesh_loss import RegularizedMeshLoss, RegularizedMeshLossHIP
    from fissure_segmentation_amd.models.folding_net import DGCNNFoldingNet
    params = list(inspect.signature(RegularizedMeshLossHIP.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("w_chamfer", 1.), ("w_edge_length", 1.), ("w_normal_consistency", 0.1),
                                                     ("w_laplacian", 0.1), ("n_samples", 2048), ("generator", None)]
    loss = RegularizedMeshLossHIP()
    assert (loss.w_chamfer, loss.w_edge_length, loss.w_normal_consistency, loss.w_laplacian, loss.n_samples) == (1, 1, .1, .1, 2048)
    with pytest.raises(NotImplementedError):          # opening the registry name is a later decision
        get_loss_fn("mesh")
    with pytest.raises(NotImplementedError):
        RegularizedMeshLoss(0., 1., 0., 0.)
    assert DGCNNFoldingNet.return_meshes is False
    net = DGCNNFoldingNet(k=8, n_embedding=64, shape_type="plane", n_input_points=64)
    assert net.return_meshes is False and "return_meshes" not in net.config
    assert "return_meshes" not in inspect.signature(DGCNNFoldingNet.__init__).parameters
    assert not any("return_meshes" in k for k in net.state_dict())
