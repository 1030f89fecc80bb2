"""Marching cubes on the GPU (csrc/marching_cubes.hip) against tests/mc_oracle.py: faces as exact integers, vertices, normals
and the gradient grid under the project's bar (dpsr_oracle.bar: 4 x the fp32 restatement's own error, floor 8 * 2^-24 x
magnitude; the magnitude is the largest coordinate for vertices, 1 for the unit normals).  Measured figures are printed as
MC_PARITY lines and kept in profiles/mc_parity.txt."""
import numpy as np
import pytest
import torch

import dpsr_oracle as do
import mc_oracle as mo

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _F():
    from fissure_segmentation_amd import functional
    return functional


def _rng(seed):
    return np.random.default_rng(seed)


def _padded(inner, value=1.0):
    out = np.full((inner.shape[0],) + tuple(s + 2 for s in inner.shape[1:]), value, np.float32)
    out[:, 1:-1, 1:-1, 1:-1] = inner
    return out


def _run(field, iso=0.0, local=True, mask=None, **kw):
    f = torch.from_numpy(np.ascontiguousarray(field)).to(_dev())
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(_dev())
    v, fc, n, nv, nf = _F().marching_cubes(f, iso, local, mask=m, **kw)
    assert v.dtype == torch.float32 and n.dtype == torch.float32 and fc.dtype == torch.int64
    assert v.shape == (sum(nv), 3) and n.shape == v.shape and fc.shape == (sum(nf), 3)
    return v.cpu().numpy(), fc.cpu().numpy(), n.cpu().numpy(), nv, nf


def _against_oracle(label, field, iso=0.0, local=True, mask=None, got=None):
    """the kernel's result on `field` equals the oracle's: counts and faces exactly, vertices and normals under the bar"""
    v, fc, n, nv, nf = got if got is not None else _run(field, iso, local, mask)
    v64, f64, n64 = mo.marching_cubes(field, iso, local, mask, np.float64)
    v32, f32, n32 = mo.marching_cubes(field, iso, local, mask, np.float32)
    assert nv == [len(x) for x in v64] and nf == [len(x) for x in f64], f"{label}: counts differ from the oracle's"
    assert np.array_equal(fc, mo.packed(f64, dtype=np.int64)), f"{label}: faces differ from the oracle's"
    assert all(np.array_equal(a, b) for a, b in zip(f32, f64))
    mag = 1.0 if local else float(max(field.shape[1:]) - 1)
    T = torch.from_numpy
    ok, msg = do.bar("MC_PARITY", f"{label} verts", T(v), T(mo.packed(v64, dtype=np.float64)), T(mo.packed(v32, dtype=np.float32)), mag)
    assert ok, msg
    ok, msg = do.bar("MC_PARITY", f"{label} normals", T(n), T(mo.packed(n64, dtype=np.float64)), T(mo.packed(n32, dtype=np.float32)), 1.0)
    assert ok, msg
    return v, fc, n, nv, nf


def _closed(faces, nv, nf):
    """every directed edge once and its reverse once, per item"""
    for f in np.split(faces, np.cumsum(nf)[:-1]):
        assert mo.directed_edge_defect(f) == (0, 0)


def test_all_256_cases():
    mag = _rng(1).uniform(0.1, 1.0, (256, 8)).astype(np.float32)
    inside = (np.arange(256)[:, None] >> np.arange(8)[None]) & 1
    field = np.where(inside == 1, -mag, mag).astype(np.float32).reshape(256, 2, 2, 2)     # corner c = x | y << 1 | z << 2
    v, fc, n, nv, nf = _against_oracle("256 cases", field)
    from fissure_segmentation_amd._mc_table import TRIANGLES
    assert nf == [len(t) for t in TRIANGLES] and sum(nf) == 820
    _against_oracle("256 cases index coords", field, local=False)


@pytest.mark.parametrize("local", (True, False))
@pytest.mark.parametrize("pad", (True, False))
def test_random_field(pad, local):
    inner = _rng(2).standard_normal((2, 9, 10, 11)).astype(np.float32)
    field = _padded(inner) if pad else inner
    v, fc, n, nv, nf = _against_oracle(f"random pad={pad} local={local}", field, local=local)
    assert min(nv) > 0
    if pad:
        _closed(fc, nv, nf)
    norm = np.linalg.norm(n, axis=1)            # unit, except where the summed area is below the 1e-6 of max(|n|, 1e-6)
    assert np.isfinite(n).all() and norm.max() < 1 + 1e-5 and np.median(norm) > 1 - 1e-5
    lo, hi = (-1.0, 1.0) if local else (0.0, float(max(field.shape[1:]) - 1))
    assert v.min() >= lo and v.max() <= hi


def test_chunk_and_word_boundaries():
    field = _rng(3).standard_normal((1, 33, 31, 70)).astype(np.float32)     # W > 64, 71610 nodes = 69.9 chunks of 1024
    _against_oracle("33x31x70", field)


def test_smooth_field_64():
    z, y, x = np.mgrid[:64, :64, :64].astype(np.float32)
    field = (np.sqrt((x - 30.3) ** 2 + (y - 33.1) ** 2 + (z - 31.7) ** 2) - 20.5 + 2 * np.sin(x / 5) * np.cos(y / 7))[None]
    v, fc, n, nv, nf = _against_oracle("smooth 64^3", field.astype(np.float32), local=False)
    _closed(fc, nv, nf)
    assert mo.euler_characteristic(fc) == 2
    assert ((v - np.array([30.3, 33.1, 31.7])) * n).sum(1).min() > 0


def test_nodes_exactly_at_the_isolevel():
    field = _rng(4).integers(-1, 2, (2, 7, 8, 9)).astype(np.float32)        # a third of the nodes are exactly 0
    v, fc, n, nv, nf = _against_oracle("nodes at the level", _padded(field))
    assert np.isfinite(v).all() and np.isfinite(n).all()
    _against_oracle("level 0.25", _padded(field * 0.25), iso=0.25)


def test_empty_items():
    inner = _rng(5).standard_normal((3, 5, 6, 7)).astype(np.float32)
    inner[1] = np.abs(inner[1]) + 1                                         # no crossing between two items with crossings
    v, fc, n, nv, nf = _against_oracle("empty item", inner)
    assert nv[1] == 0 and nf[1] == 0 and nv[0] > 0 and nv[2] > 0
    v, fc, n, nv, nf = _run(np.ones((2, 4, 5, 6), np.float32))
    assert nv == [0, 0] and nf == [0, 0] and v.shape == (0, 3) and fc.shape == (0, 3) and n.shape == (0, 3)


@pytest.mark.parametrize("dtype", (torch.float64, torch.bfloat16))
def test_other_float_types_are_converted_to_fp32(dtype):
    f = torch.from_numpy(_rng(6).standard_normal((2, 6, 7, 8))).to(_dev()).to(dtype)
    a = _F().marching_cubes(f)
    b = _F().marching_cubes(f.to(torch.float32))
    assert a[3:] == b[3:] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_non_finite_values():
    field = _rng(7).standard_normal((2, 5, 6, 7)).astype(np.float32)
    field[1, 2, 3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        _run(field)
    v, fc, n, nv, nf = _run(field, validate=False)                          # NaN is outside; the vertices on its edges are NaN
    f64 = mo.marching_cubes(field)[1]
    assert nf == [len(f) for f in f64] and np.array_equal(fc, mo.packed(f64, dtype=np.int64))
    nb = [field[1, 2 + dz, 3 + dy, 4 + dx] for dz, dy, dx in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))]
    assert np.isfinite(v[:nv[0]]).all() and np.isnan(v[nv[0]:]).any(1).sum() == sum(x < 0 for x in nb) > 0
    field[1, 2, 3, 4] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        _run(field)


def test_mask():
    field = _padded(_rng(8).standard_normal((2, 9, 10, 11)).astype(np.float32))
    mask = np.ones(field.shape, np.uint8)
    mask[:, :, :, 7:] = 0                                                   # cuts the surface
    mask[0, 3:5, 4:6, 2:4] = 0
    v, fc, n, nv, nf = _against_oracle("mask", field, mask=mask)
    for f, k in zip(np.split(fc, np.cumsum(nf)[:-1]), nv):
        assert np.array_equal(np.unique(f), np.arange(k)), "an unreferenced vertex"
    full = _run(field)
    assert all(a < b for a, b in zip(nf, full[4]))
    shared = _run(field, mask=mask[1])                                      # one (D, H, W) mask for all items
    per_item = _run(field, mask=np.stack([mask[1], mask[1]]))
    assert shared[3:] == per_item[3:] and all(np.array_equal(a, b) for a, b in zip(shared[:3], per_item[:3]))


def test_same_bits_every_run_and_in_any_batch():
    field = _rng(9).standard_normal((3, 12, 13, 14)).astype(np.float32)
    a, b = _run(field), _run(field)
    assert a[3:] == b[3:] and all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32)
                                                 if y.dtype == np.float32 else y) for x, y in zip(a[:3], b[:3]))
    alone = _run(field[1:2])
    v0, f0 = sum(a[3][:1]), sum(a[4][:1])
    assert alone[3] == a[3][1:2] and alone[4] == a[4][1:2]
    assert np.array_equal(alone[0].view(np.uint32), a[0][v0:v0 + alone[3][0]].view(np.uint32))
    assert np.array_equal(alone[2].view(np.uint32), a[2][v0:v0 + alone[3][0]].view(np.uint32))
    assert np.array_equal(alone[1], a[1][f0:f0 + alone[4][0]])


def _oracle_grad(field, G, dtype):
    """-(G . n) at the oracle's vertices, splatted in the 'torch' convention -> (B, D, H, W)"""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    vs, _, ns = mo.marching_cubes(field, 0.0, True, None, dtype)
    B, N = len(vs), G.shape[1]
    vals, pts = torch.zeros(B, 1, N, dtype=tdt), torch.zeros(B, N, 3, dtype=tdt)
    for b, (v, n) in enumerate(zip(vs, ns)):
        vals[b, 0, :len(v)] = -(torch.from_numpy(G[b, :len(v)].astype(dtype)) * torch.from_numpy(n)).sum(-1)
        pts[b, :len(v)] = torch.from_numpy(v)
    return do.splat(vals, pts, tuple(field.shape[1:]), "torch")[:, 0]


def test_backward_splats_minus_g_dot_n():
    from fissure_segmentation_amd.models.dpsr_utils import DifferentiableMarchingCubes
    field = _rng(10).standard_normal((2, 8, 10, 12)).astype(np.float32)
    field[1, :, :, 6:] = np.abs(field[1, :, :, 6:]) + 0.5                   # unequal vertex counts
    psr = torch.from_numpy(field).to(_dev()).requires_grad_(True)
    verts, faces, normals = DifferentiableMarchingCubes.apply(psr)
    nv = [len(v) for v in mo.marching_cubes(field, 0.0, True)[0]]
    assert nv[0] != nv[1] and verts.shape == (2, max(nv), 3) and normals.shape == verts.shape and faces.shape[0] == 2
    assert int((faces[1] < 0).all(-1).sum()) == faces.shape[1] - len(mo.marching_cubes(field, 0.0, True)[1][1])
    assert not verts[1, nv[1]:].any() and not normals[1, nv[1]:].any()
    G = _rng(11).standard_normal(tuple(verts.shape)).astype(np.float32)
    got, = torch.autograd.grad((verts * torch.from_numpy(G).to(_dev())).sum() + normals.sum(), psr)
    assert got.shape == psr.shape
    want64, want32 = _oracle_grad(field, G, np.float64), _oracle_grad(field, G, np.float32)
    ok, msg = do.bar("MC_PARITY", "backward grid", got, want64, want32)
    assert ok, msg


def test_backward_of_an_empty_batch_is_zero():
    from fissure_segmentation_amd.models.dpsr_utils import DifferentiableMarchingCubes
    psr = torch.ones(2, 4, 5, 6, device=_dev(), requires_grad=True)
    verts, faces, normals = DifferentiableMarchingCubes.apply(psr)
    assert verts.shape == (2, 0, 3) and faces.shape == (2, 0, 3) and normals.shape == (2, 0, 3)
    got, = torch.autograd.grad(verts.sum(), psr)
    assert got.shape == psr.shape and not got.any()


def test_softmesh_meshes():
    from fissure_segmentation_amd.mesh import Meshes
    from fissure_segmentation_amd.models.seg_logits_to_mesh import SoftMesh
    m = {k: v.to(_dev()) for k, v in do.softmesh_case().items()}
    sm = SoftMesh(do.SMOOTH_SIGMA, do.RES, do.SIG).to(_dev())
    lg = do.leaf(m["logits"])
    meshes = sm.meshes(lg, m["coords"])
    assert isinstance(meshes, Meshes) and len(meshes) == 4
    psr = sm.psr_grid(lg, m["coords"]).detach().cpu().numpy()
    nv, nf = meshes.num_verts_per_mesh().tolist(), meshes.num_faces_per_mesh().tolist()
    assert min(nv) > 0 and min(nf) > 0
    got = (meshes.verts_packed().detach().cpu().numpy(), torch.cat(meshes.faces_list()).cpu().numpy(),
           meshes.verts_normals_packed().detach().cpu().numpy(), nv, nf)
    _against_oracle("SoftMesh.meshes", psr, got=got)
    g, = torch.autograd.grad(meshes.verts_packed().square().sum(), lg)
    assert g.shape == lg.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    with pytest.raises(NotImplementedError, match="marching cubes"):
        sm(lg, m["coords"])


def test_dpsrnet2_and_dpsrloss_one_step():
    from fissure_segmentation_amd.losses.dpsr_loss import DPSRLoss
    from fissure_segmentation_amd.mesh import Meshes
    from fissure_segmentation_amd.models.seg_logits_to_mesh import DPSRNet2
    torch.manual_seed(0)
    net = DPSRNet2("DGCNN", k=8, in_features=3, num_classes=4, normals_smoothing_sigma=do.SMOOTH_SIGMA, dpsr_res=do.RES,
                   dpsr_sigma=do.SIG).to(_dev()).train()
    g = torch.Generator().manual_seed(13)
    x = (torch.rand(2, 3, 256, generator=g) * 0.25 + 0.75).to(_dev())       # where the two conventions of SoftMesh overlap
    seg, meshes = net(x)
    assert seg.shape == (2, 4, 256) and len(meshes) == 6 and min(meshes.num_verts_per_mesh().tolist()) > 0
    z, y, xx = np.mgrid[:12, :12, :12].astype(np.float32)
    ball = torch.from_numpy(np.sqrt((xx - 5.5) ** 2 + (y - 5.5) ** 2 + (z - 5.5) ** 2) - 4)[None].to(_dev())
    v, f, n, _, _ = _F().marching_cubes(ball)
    target = (torch.randint(0, 4, (2, 256), generator=g).to(_dev()), Meshes([v] * 6, [f] * 6, [n] * 6))
    loss, parts = DPSRLoss(None)((seg, meshes), target, current_epoch_fraction=0.5)
    assert set(parts) == {"Segmentation", "Chamfer"} and float(parts["Chamfer"]) > 0
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in net.seg_net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    early, parts = DPSRLoss(None)((seg.detach(), meshes), target, current_epoch_fraction=0.0)
    assert float(parts["Chamfer"]) == 0 and float(early) == float(parts["Segmentation"])
    with pytest.raises(NotImplementedError, match="never defines"):
        net.predict_full_pointcloud(x)


def test_labels_equal_the_float_path():
    lab = _rng(14).integers(0, 5, (12, 14, 16)).astype(np.int64)
    lab[3:9, 4:10, 5:11] = 2                                                # a solid block among the noise
    t = torch.from_numpy(lab).to(_dev())
    got = _F().marching_cubes_labels(t, 1, 3)
    field = torch.stack([(t != lb).float() for lb in (1, 2, 3)])
    want = _F().marching_cubes(field, 0.5, return_local_coords=False)
    assert got[3:] == want[3:] and min(got[3]) > 0
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
    frac = got[0] - got[0].floor()
    assert bool(((frac == 0) | (frac == 0.5)).all())                       # every vertex is an edge midpoint
    mask = torch.ones_like(t, dtype=torch.bool)
    mask[:, :, 8:] = False
    gm = _F().marching_cubes_labels(t, 1, 3, mask=mask)
    wm = _F().marching_cubes(field, 0.5, return_local_coords=False, mask=mask)
    assert gm[3:] == wm[3:] and all(torch.equal(a, b) for a, b in zip(gm[:3], wm[:3])) and sum(gm[4]) < sum(got[4])


def test_compute_surface_mesh_applies_spacing_in_xyz():
    from fissure_segmentation_amd.data_processing.find_lobes import compute_surface_mesh_marching_cubes
    lab = np.zeros((12, 14, 16), np.int64)
    lab[2:5, 3:9, 4:12] = 1          # z 2..4, y 3..8, x 4..11
    lab[7:10, 3:9, 4:12] = 2
    t = torch.from_numpy(lab).to(_dev())
    sp = (0.5, 2.0, 4.0)             # powers of two: the scaled coordinates are exact
    meshes = compute_surface_mesh_marching_cubes(t, spacing=sp)
    unit = compute_surface_mesh_marching_cubes(t, max_label=2)
    assert len(meshes) == 2 and len(unit) == 2 and all(len(m) == 1 for m in meshes)
    for m, u in zip(meshes, unit):
        assert torch.equal(m.faces_list()[0], u.faces_list()[0])
        assert torch.equal(m.verts_list()[0], u.verts_list()[0] * torch.tensor(sp, device=_dev()))
    v = unit[0].verts_list()[0]
    assert v.min(0).values.tolist() == [3.5, 2.5, 1.5] and v.max(0).values.tolist() == [11.5, 8.5, 4.5]      # (x, y, z)
    f = unit[0].faces_list()[0].cpu().numpy()
    assert mo.directed_edge_defect(f) == (0, 0) and mo.euler_characteristic(f) == 2
    c = torch.tensor([7.5, 5.5, 3.0], device=_dev())
    assert float(((v - c) * unit[0].verts_normals_list()[0]).sum(1).min()) > 0                               # out of the object
    assert mo.signed_volume(v.cpu().numpy(), f) > 0
