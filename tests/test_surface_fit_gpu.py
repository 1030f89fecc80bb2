"""GPU tests of the surface-fitting feature against tests/surface_fit_oracle.py (numpy + scipy.sparse.csgraph, pinned by
tests/test_surface_fit_cpu.py) and, end to end, against the fp64 pipeline of tests/dpsr_oracle.py + tests/mc_oracle.py.

What is exact is compared bit for bit: orientation signs and component ids (on inputs whose dot products are exact in fp32, so the
forest is unique whatever the evaluation order), cluster numbers and counts, distinct-vertex counts, compacted vertices and faces.
Areas are held to 4 x the error of the fp32 restatement against the fp64 oracle, floor 4.8e-7 relative.  The end-to-end bar is
the fp64 oracle pipeline's own largest distance to the analytic surface plus one grid cell.  Every case prints its figures."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpsr_oracle
import mc_oracle
import normals_oracle
import surface_fit_oracle as so
from conftest import ROOT

pytestmark = pytest.mark.gpu

MM, CENTRE = 50.0, np.array([150.0, 110.0, 90.0])       # the end-to-end ellipsoid: semi-axes 50, 35, 20 "mm", off-centre
MASK_SPACING = (1.5, 1.0, 0.8)
DEPTH, FIT_SCALE, SIGMA = 5, 1.1, 10


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- orientation, exact
def _integer_case(seed, sizes):
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    normals = rng.integers(-4, 5, (n, 3))
    while (zero := (normals == 0).all(1)).any():
        normals[zero] = rng.integers(-4, 5, (int(zero.sum()), 3))
    return xyz, (normals / 8).astype(np.float32), np.cumsum(sizes).astype(np.int32)


@pytest.mark.parametrize("sizes,K", [((257, 64, 1), 8), ((235, 40, 25), 64)], ids=["257-64-1_K8", "235-40-25_K64"])
def test_orientation_equals_the_oracle_bit_for_bit(fsg, device, sizes, K):
    """normals are integer vectors / 8: every product and sum of a dot product is exact in fp32, so the weights, the keys and
    with them the forest are the same in any evaluation order.  With K = 64 the segments of 40 and 25 points clamp k_s."""
    F = fsg.functional
    xyz, normals, off = _integer_case(11 + K, sizes)
    x, nr, o = G(xyz, device), G(normals, device), G(off, device)
    idx = F.knn_segment(K, x, x, o, o)[0]
    want = so.orient(xyz, normals, N(idx), off)
    for given in (idx, None):
        out, signs, comp = F.orient_normals_consistent(x, nr, o, K, idx=given)
        assert signs.dtype == torch.int8 and comp.dtype == torch.int32 and out.dtype == torch.float32
        assert np.array_equal(N(signs), want["signs"]) and np.array_equal(N(comp), want["comp"])
        assert np.array_equal(bits(N(out)), bits(want["oriented"]))
    ncomp = len(np.unique(want["comp"]))
    print(f"\norientation {sizes} K={K}: {len(want['forest'])} forest edges of {len(want['edges'][0])}, {ncomp} components, "
          f"{int((want['signs'] < 0).sum())} flipped")
    assert ncomp >= 3 and 0 < (want["signs"] < 0).sum() < sum(sizes)


def test_orientation_of_nothing_and_of_single_points(fsg, device):
    F = fsg.functional
    out, signs, comp = F.orient_normals_consistent(torch.zeros(0, 3, device=device), torch.zeros(0, 3, device=device),
                                                   torch.zeros(1, dtype=torch.int32, device=device), 4)
    assert out.shape == (0, 3) and signs.shape == (0,) and comp.shape == (0,)
    nr = G(np.array([[0, 0, -1.0], [0, 1.0, 0.5], [1.0, 0, -0.0]], np.float32), device)
    out, signs, comp = F.orient_normals_consistent(torch.rand(3, 3, device=device), nr, G(np.array([1, 1, 2, 3], np.int32), device), 4)
    assert N(signs).tolist() == [-1, 1, 1] and N(comp).tolist() == [0, 1, 2]
    assert np.array_equal(bits(N(out)), bits(np.array([[-0.0, -0.0, 1.0], [0, 1.0, 0.5], [1.0, 0, -0.0]], np.float32)))


# ---------------------------------------------------------------- orientation, properties
@pytest.mark.parametrize("cloud", ["ellipsoid", "sheet"])
def test_orientation_properties(fsg, device, cloud):
    F = fsg.functional
    xyz, ana = so.ellipsoid(2048, 1) if cloud == "ellipsoid" else so.wavy_sheet(2048, 1)
    off = np.array([2048], np.int32)
    x, o = G(xyz, device), G(off, device)
    idx = F.knn_segment(16, x, x, o, o)[0]
    # the precondition, on the oracle and on the very lists the kernel reads: one component
    u, v, _, _, _ = so.graph_edges(np.ones((2048, 3), np.float32), N(idx), off)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    assert connected_components(coo_matrix((np.ones(len(u)), (u, v)), shape=(2048, 2048)), directed=False)[0] == 1
    normals = F._pcl_packed(x, o, 16, False, idx, False, False)[0]
    out, signs, comp = F.orient_normals_consistent(x, normals, o, 16, idx=idx)
    side = (N(out).astype(np.float64) * ana).sum(1)
    print(f"\n{cloud}: {int((N(signs) < 0).sum())} of 2048 flipped, min cos to the analytic normal {side.min():.4f}")
    assert (N(comp) == 0).all()
    assert (side > 0).all()                                   # outward / upward: the member of largest z has n_z >= 0
    # flipping a random half of the inputs gives identical bits (the Jacobi solver's own signs can be consistent already, as on
    # the sheet, where its normals all come out upward: the flipped run is the one with arbitrary signs)
    flip = G(np.random.default_rng(5).random(2048) < 0.5, device)
    again, signs2, _ = F.orient_normals_consistent(x, torch.where(flip[:, None], -normals, normals), o, 16, idx=idx)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    assert torch.equal(signs2, torch.where(flip, -signs, signs))
    # alone and inside a batch: identical bits
    other = G(so.ellipsoid(300, 9)[0] + np.float32(3), device)
    xb = torch.cat([other, x, other[:77]])
    ob = G(np.array([300, 2348, 2425], np.int32), device)
    idxb = F.knn_segment(16, xb, xb, ob, ob)[0]
    assert torch.equal(idxb[300:2348] - 300, idx)
    nb = F._pcl_packed(xb, ob, 16, False, idxb, False, False)[0]
    outb, signsb, compb = F.orient_normals_consistent(xb, nb, ob, 16, idx=idxb)
    assert torch.equal(outb[300:2348].view(torch.int32), out.view(torch.int32)) and torch.equal(signsb[300:2348], signs)
    assert torch.equal(compb[300:2348], comp + 300)


# ---------------------------------------------------------------- face clusters, statistics, compaction
@pytest.fixture(scope="module")
def blobs(fsg, device):
    """the batch every clean-up test shares: marching cubes of the blob field (in index units), the hand-made fan, an empty mesh,
    and the oracle's view of them; computed once and only read"""
    F = fsg.functional
    from fissure_segmentation_amd.mesh import Meshes
    verts, faces, normals, nv, nf = F.marching_cubes(G(so.blob_field(), device)[None], 0.0, return_local_coords=False)
    fan_v, fan_f = so.fan_mesh()
    meshes = Meshes([verts, G(fan_v, device), verts[:0], verts + 0.25],
                    [faces, G(fan_f, device), faces[:0], faces], [normals, G(fan_v, device), normals[:0], normals])
    host = [(N(v), N(f)) for v, f in zip(meshes.verts_list(), meshes.faces_list())]
    want = [so.face_clusters(f) for _, f in host]
    return SimpleNamespace(meshes=meshes, host=host, clusters=[w[0] for w in want], counts=[w[1] for w in want],
                           normals=[N(n) for n in meshes.verts_normals_list()])


def test_face_clusters_equal_the_oracle(fsg, device, blobs):
    F = fsg.functional
    clusters, counts = F.mesh_face_components(blobs.meshes)
    assert clusters.dtype == torch.int32 and counts.dtype == torch.int64 and counts.is_cuda
    print(f"\nface clusters: {[len(f) for _, f in blobs.host]} faces -> {blobs.counts} clusters")
    assert N(counts).tolist() == blobs.counts == [blobs.counts[0], 4, 0, blobs.counts[0]] and blobs.counts[0] in (4, 5)
    assert np.array_equal(N(clusters), np.concatenate(blobs.clusters))
    single, c1 = F.mesh_face_components((blobs.meshes.verts_list()[1], blobs.meshes.faces_list()[1]))
    assert N(single).tolist() == [0, 1, 0, 2, 0, 3] and N(c1).tolist() == [4]


def test_cluster_statistics(fsg, device, blobs):
    F = fsg.functional
    clusters = G(np.concatenate(blobs.clusters), device)
    area, num, vsum, counts = F.mesh_component_stats(blobs.meshes, clusters)
    assert counts == blobs.counts and area.dtype == torch.float64 and vsum.dtype == torch.float64 and num.dtype == torch.int64
    area, num, vsum = N(area), N(num), N(vsum)
    at = 0
    for m, ((v, f), cl) in enumerate(zip(blobs.host, blobs.clusters)):
        if len(f) == 0:
            continue
        a64, n64, s64 = so.cluster_stats(v, f, cl, np.float64)
        a32, _, s32 = so.cluster_stats(v, f, cl, np.float32)
        c = len(a64)
        got_a, got_n, got_s = area[at:at + c], num[at:at + c], vsum[at:at + c]
        at += c
        bar = np.maximum(4 * np.abs(a32.astype(np.float64) - a64), 4.8e-7 * a64)
        bar_s = np.maximum(4 * np.abs(s32.astype(np.float64) - s64), 4.8e-7 * np.abs(s64).max())
        print(f"mesh {m}: area error {np.abs(got_a - a64).max():.3e} (bar {bar.min():.3e}), vertex-sum error "
              f"{np.abs(got_s - s64).max():.3e} (bar {bar_s.min():.3e}), distinct vertices {got_n.tolist()}")
        assert np.array_equal(got_n, n64)
        assert (np.abs(got_a - a64) <= bar).all() and (np.abs(got_s - s64) <= bar_s).all()
    assert at == len(area)


def _check_meshes(got, want_v, want_f, want_n=None):
    for m, (v, f) in enumerate(zip(got.verts_list(), got.faces_list())):
        assert f.dtype == torch.int64 and np.array_equal(N(f), want_f[m]), m
        assert np.array_equal(bits(N(v)), bits(want_v[m].astype(np.float32))), m
        if want_n is not None:
            assert np.array_equal(bits(N(got.verts_normals_list()[m])), bits(want_n[m].astype(np.float32))), m


def test_compaction_equals_the_oracle(fsg, device, blobs):
    """a box with a vertex exactly on its face, a mask with coordinates beyond the volume (clamped) and below zero (dropped), a
    cluster choice, and a mesh that becomes empty"""
    F = fsg.functional
    v0 = blobs.host[0][0]
    on_face = v0[np.argmin(np.abs(v0[:, 0] - 7.0))]                                   # a vertex of mesh 0: the box ends ON it
    box = np.array([[2.0, 1.5, 3.0], [float(on_face[0]), 17.0, 19.5]], np.float32)
    wide = np.array([[-100.0, -100.0, -100.0], [float(on_face[0] - np.float32(3.0)), 100.0, 100.0]], np.float32)
    mask = np.random.default_rng(2).random((10, 12, 9)) < 0.7                          # D, H, W: smaller than the meshes' extent
    spacing = (1.5, 1.25, 2.0)
    shifted = [(v - np.float32(3.0) if m == 0 else v, f) for m, (v, f) in enumerate(blobs.host)]      # mesh 0 reaches below 0
    from fissure_segmentation_amd.mesh import Meshes
    meshes = Meshes([G(v, device) for v, _ in shifted], [G(f, device) for _, f in shifted], [G(n, device) for n in blobs.normals])
    assert shifted[0][0].min() < 0 and shifted[3][0][:, 0].max() / spacing[0] > 9
    face_keep = [cl == (1 if len(cl) else 0) for cl in blobs.clusters]                 # cluster 1 of every mesh
    at_face = shifted[0][0][:, 0] == wide[1, 0]
    assert so.keep_flags(shifted[0][0], wide)[at_face].all() and at_face.any()        # exactly on the box face: kept
    cases = {"box": dict(box=wide), "mask": dict(mask=mask, spacing=spacing),
             "box+mask": dict(box=box, mask=mask, spacing=spacing), "cluster": dict(face_keep=face_keep, drop_unreferenced=True),
             "all": dict(box=wide, mask=mask, spacing=spacing, face_keep=[cl == 0 for cl in blobs.clusters], drop_unreferenced=True),
             "nothing left": dict(box=np.array([[100.0, 100, 100], [101, 101, 101]], np.float32), drop_unreferenced=True)}
    for name, kw in cases.items():
        want = []
        for m, (v, f) in enumerate(shifted):
            keep = so.keep_flags(v, kw.get("box"), kw.get("mask"), kw.get("spacing"))
            want.append(so.compact(v, f, keep, kw["face_keep"][m] if "face_keep" in kw else None, kw.get("drop_unreferenced", False),
                                   blobs.normals[m]))
        args = dict(kw)
        for k in ("box", "mask"):
            if k in args:
                args[k] = G(args[k], device)
        if "face_keep" in args:
            args["face_keep"] = G(np.concatenate(args["face_keep"]), device)
        got = F.mesh_remove_vertices(meshes, **args)
        print(f"{name}: vertices {[len(v) for v, _ in shifted]} -> {[len(w[0]) for w in want]}, faces -> {[len(w[1]) for w in want]}")
        assert len(got) == 4
        _check_meshes(got, [w[0] for w in want], [w[1] for w in want], [w[2] for w in want])
        if name == "nothing left":
            assert all(len(w[0]) == 0 and len(w[1]) == 0 for w in want)
        elif name in ("box", "mask", "box+mask"):
            assert 0 < len(want[0][0]) < len(shifted[0][0]) and 0 < len(want[0][1])
    keep = np.concatenate([np.arange(len(v)) % 3 != 0 for v, _ in shifted])
    got = F.mesh_remove_vertices(meshes, keep=G(keep, device))
    at = 0
    for m, (v, f) in enumerate(shifted):
        wv, wf = so.compact(v, f, keep[at:at + len(v)])
        at += len(v)
        assert np.array_equal(N(got.verts_list()[m]), wv) and np.array_equal(N(got.faces_list()[m]), wf)


def test_mask_out_verts_from_mesh(fsg, device, blobs):
    from fissure_segmentation_amd.utils import general_utils as gu
    mask = np.random.default_rng(4).random((12, 20, 14)) < 0.8
    spacing = torch.tensor([2.0, 1.0, 2.0])
    got = gu.mask_out_verts_from_mesh(blobs.meshes, G(mask, device), spacing)
    want = [so.compact(v, f, so.keep_flags(v, None, mask, (2.0, 1.0, 2.0))) for v, f in blobs.host]
    _check_meshes(got, [w[0] for w in want], [w[1] for w in want])
    v, f = blobs.host[0]
    one = gu.mask_out_verts_from_mesh((v, f), mask, spacing)                          # host arrays: to the current GPU
    _check_meshes(one, [want[0][0]], [want[0][1]])


@pytest.mark.parametrize("right,center_x", [(None, None), (True, 13.0), (False, 13.0), (True, -5.0), (False, 99.0), (True, None)],
                         ids=["plain", "right", "left", "none-right-of", "none-left-of", "no-centre"])
def test_remove_all_but_biggest_component(fsg, device, blobs, right, center_x):
    """center_x = 13 lies between the blobs at x ~ 6 / 8 and those at x ~ 20; -5 and 99 leave no cluster on the wanted side"""
    from fissure_segmentation_amd.utils import general_utils as gu
    got = gu.remove_all_but_biggest_component(blobs.meshes, right=right, center_x=center_x)
    want_v, want_f, chosen = [], [], []
    for v, f in blobs.host:
        if len(f) == 0:
            want_v.append(v), want_f.append(f), chosen.append(None)
            continue
        k, cl, _ = so.biggest_component(v, f, right, center_x)
        wv, wf = so.compact(v, f, np.ones(len(v), bool), cl == k, True)
        want_v.append(wv), want_f.append(wf), chosen.append(k)
    print(f"\nright={right} center_x={center_x}: clusters chosen {chosen}, faces kept {[len(f) for f in want_f]}")
    _check_meshes(got, want_v, want_f)
    if center_x == 13.0:
        cx = [N(got.verts_list()[m])[:, 0].mean() for m in (0, 3)]
        assert (cx[0] < 13.0) == bool(right) and (cx[1] < 13.0) == bool(right)
    per_mesh = gu.remove_all_but_biggest_component(blobs.meshes, right=[True, False, True, False], center_x=13.0)
    for m, r in enumerate((True, False, True, False)):
        if len(blobs.host[m][1]):
            k, cl, _ = so.biggest_component(*blobs.host[m], r, 13.0)
            assert np.array_equal(N(per_mesh.faces_list()[m]), so.compact(*blobs.host[m], np.ones(len(blobs.host[m][0]), bool), cl == k, True)[1])


# ---------------------------------------------------------------- end to end
def _oracle_pipeline(xyz, normals):
    """the fp64 pipeline on given normals: bounding cube, DPSR, marching cubes, back to world -> verts, faces, cube side"""
    res = (2 ** DEPTH,) * 3
    lo, hi = xyz.min(0), xyz.max(0)
    centre = (lo + hi) / np.float32(2)
    half = (hi - lo).max() * np.float32(FIT_SCALE / 2)
    V = ((xyz - centre) / half)[:, ::-1].copy()                                       # the grid's axes are (z, y, x)
    phi = dpsr_oracle.dpsr(torch.from_numpy(V).double()[None], torch.from_numpy(normals[:, ::-1].copy()).double()[None], res=res,
                           sig=SIGMA)[0]
    v, f, _ = mc_oracle.marching_cubes_item(phi.float().numpy(), 0.0, True, None, np.float64)
    return v * float(half) + centre.astype(np.float64), f, 2 * float(half)


def _biggest(v, f):
    k, cl, c = so.biggest_component(v, f)
    return so.compact(v, f, np.ones(len(v), bool), cl == k, True) + (c,)


def _world_cloud(n, seed):
    unit, _ = so.ellipsoid(n, seed)
    return (unit.astype(np.float64) * MM + CENTRE).astype(np.float32)


def test_pointcloud_surface_fitting_end_to_end(fsg, device):
    """GPU: 1500 points on the ellipsoid with semi-axes 50, 35, 20 centred at (150, 110, 90), depth 5 (cube side 110, cell 3.44).
    Figures of the fp64 oracle pipeline (CPU, seed 1): largest distance to the analytic surface 3.94 with the oracle's oriented
    normals, 43.6 with the unoriented PCA normals -- the bar is 3.94 + 3.44 = 7.38, so the orientation step is what decides."""
    from fissure_segmentation_amd.data_processing import pointcloud_surface_fitting as sf
    from fissure_segmentation_amd.utils import general_utils as gu
    xyz = _world_cloud(1500, 1)
    off = np.array([1500], np.int32)
    axes = np.array(so.AXES) * MM
    idx30 = so.knn(xyz, off, 30)
    raw = normals_oracle.frames(xyz, 30, idx=idx30.astype(np.int64), dtype=np.float64, disambiguate=False)["normals"].astype(np.float32)
    oriented = so.orient(xyz, raw, so.knn(xyz, off, 64), off)["oriented"]
    ov, of, side = _oracle_pipeline(xyz, oriented)
    ov, of, oc = _biggest(ov, of)
    oracle_dist = so.ellipsoid_distance(ov, axes, CENTRE).max()
    cell = side / 2 ** DEPTH
    bar = oracle_dist + cell
    uv, uf, _ = _oracle_pipeline(xyz, raw)
    uv, uf, _ = _biggest(uv, uf)
    unoriented_dist = so.ellipsoid_distance(uv, axes, CENTRE).max()
    assert unoriented_dist > bar                              # without the orientation step the same solver misses the bar

    mask = torch.ones(160, 160, 160, dtype=torch.bool, device=device)                 # (D, H, W): covers the cloud at MASK_SPACING
    mesh = sf.pointcloud_surface_fitting(xyz, crop_to_bbox=False, mask=mask, spacing=MASK_SPACING, depth=DEPTH, scale=FIT_SCALE)
    assert len(mesh) == 1 and mesh.device.type == "cuda"
    plain = sf.pointcloud_surface_fitting(G(xyz, device), depth=DEPTH)
    assert torch.equal(plain.verts_packed(), mesh.verts_packed()) and torch.equal(plain.faces_packed(), mesh.faces_packed())
    clean = gu.remove_all_but_biggest_component(mesh)
    v, f = N(clean.verts_list()[0]).astype(np.float64), N(clean.faces_list()[0])
    clusters, c = so.face_clusters(f)
    got_dist = so.ellipsoid_distance(v, axes, CENTRE).max()
    lines = [f"pointcloud_surface_fitting, 1500 points on an ellipsoid (semi-axes {axes.tolist()}), depth {DEPTH}, cell {cell:.4f}",
             f"  largest vertex distance to the analytic surface: GPU {got_dist:.4f}, fp64 oracle pipeline {oracle_dist:.4f}, "
             f"bar {bar:.4f}", f"  the oracle pipeline on unoriented normals: {unoriented_dist:.4f}",
             f"  GPU mesh: {len(v)} vertices, {len(f)} faces, {c} cluster(s), Euler characteristic {mc_oracle.euler_characteristic(f)}; "
             f"oracle mesh: {len(ov)} vertices, {len(of)} faces, {oc} cluster(s) before the clean-up"]
    print("\n" + "\n".join(lines))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "surface_fit_parity.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    assert got_dist <= bar
    assert c == 1 and mc_oracle.directed_edge_defect(f) == (0, 0) and mc_oracle.euler_characteristic(f) == 2
    cropped = sf.pointcloud_surface_fitting(xyz, crop_to_bbox=True, depth=DEPTH)
    cv = N(cropped.verts_packed())
    assert 0 < len(cv) <= len(N(mesh.verts_packed())) and (cv >= xyz.min(0)).all() and (cv <= xyz.max(0)).all()


def test_fit_label_surfaces_equals_the_single_calls(fsg, device):
    from fissure_segmentation_amd.data_processing import pointcloud_surface_fitting as sf
    a, b = _world_cloud(1500, 1), (_world_cloud(900, 2) - CENTRE.astype(np.float32)) * np.float32(0.6) + np.float32(60.0)
    rng = np.random.default_rng(6)
    pts = np.concatenate([a, b, rng.normal(size=(5, 3)).astype(np.float32)])
    labels = np.concatenate([np.full(1500, 1), np.full(900, 2), [0, 0, 3, 3, 7]])      # label 3: two points, no surface
    order = rng.permutation(len(pts))
    both = sf.fit_label_surfaces(pts[order], labels[order], 3, depth=DEPTH, crop_to_bbox=True)
    assert len(both) == 3 and both._nv[2] == 0 and both._nf[2] == 0
    for m, cloud in enumerate((a, b)):
        alone = sf.pointcloud_surface_fitting(pts[order][labels[order] == m + 1], depth=DEPTH, crop_to_bbox=True)
        print(f"label {m + 1}: {alone._nv[0]} vertices, {alone._nf[0]} faces alone; {both._nv[m]}, {both._nf[m]} in the batch")
        assert alone._nv[0] > 100
        assert torch.equal(alone.verts_list()[0].view(torch.int32), both.verts_list()[m].view(torch.int32))
        assert torch.equal(alone.faces_list()[0], both.faces_list()[m])
        assert torch.equal(alone.verts_normals_list()[0].view(torch.int32), both.verts_normals_list()[m].view(torch.int32))
