"""GPU tests of the point-to-mesh kernel (fsg_point_mesh_dist_f32) and of fissure_segmentation_amd.metrics against the fp64
oracle of tests/metrics_oracle.py.  The bar on every distance is the project's parity bar, 1e-4 absolute on unit-scale
coordinates.  open3d is not available, so parity with the reference's own implementation is not pinned; the oracle is pinned
by the closed forms of tests/test_metrics_cpu.py, which run through the kernel here as well."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import metrics_oracle as mo
from golden_util import cloud, fill_state_dict
from test_metrics_cpu import closed_form_cases, degenerate_cases

pytestmark = pytest.mark.gpu

BAR = 1e-4            # distances, absolute
ON_FACE = 1e-5        # barycentric coordinates of `closest` within [0, 1], and its distance to the face's plane


@pytest.fixture(scope="module")
def fsg():
    import fissure_segmentation_amd as pkg
    return pkg


def G(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def _shape_case(name):
    """-> pts (B,P,3), verts (B,V,3) fp32, faces (F,3) int64"""
    if name == "pcae_2x2025x3872":       # the PC-AE mesh of n_input_points=2048 (45 x 45 vertices) against itself perturbed
        verts, faces = mo.height_field_mesh(1301, 2, 45)
        pts = (verts + 0.01 * np.random.default_rng(1302).standard_normal(verts.shape)).astype(np.float32)
    elif name == "grid64_1x20000x7938":
        verts, faces = mo.height_field_mesh(1303, 1, 64)
        pts = mo.height_field_points(1304, 1, 20000)
    else:                                # neither P nor F a multiple of a tile
        verts, faces = mo.height_field_mesh(1305, 3, 3)
        faces = faces[:7]
        pts = mo.height_field_points(1306, 3, 131)
    return pts, verts, faces


@pytest.mark.parametrize("name", ["pcae_2x2025x3872", "grid64_1x20000x7938", "odd_3x131x7"])
def test_kernel_vs_fp64_oracle(fsg, device, name):
    pts, verts, faces = _shape_case(name)
    B, P, F = pts.shape[0], pts.shape[1], len(faces)
    dist, face, closest = fsg.functional.point_mesh_distance(G(pts, device), G(verts, device), G(faces, device), return_face=True,
                                                             return_closest=True)
    assert dist.shape == (B, P) and dist.dtype == torch.float32 and not dist.requires_grad
    assert face.shape == (B, P) and face.dtype == torch.int32 and closest.shape == (B, P, 3)
    dist, face, closest = N(dist), N(face), N(closest)
    assert np.isfinite(dist).all() and face.min() >= 0 and face.max() < F
    err = err32 = err_face = 0.0
    sub = slice(0, 2000)                 # the fp32 restatement emulates every fma in fp64: a subset of the queries is enough
    for b in range(B):
        want = mo.point_mesh_dist2(pts[b], verts[b], faces)[0].sqrt().numpy()
        r32 = mo.kernel_order_dist2(pts[b][sub], verts[b], faces).sqrt().numpy()
        err = max(err, float(np.abs(dist[b] - want).max()))
        err32 = max(err32, float(np.abs(r32 - want[sub]).max()))
        # the face: several faces are equally near a query whose closest point is on a shared edge or vertex, so the index is not
        # compared; the fp64 distance to the RETURNED face has to be the fp64 minimum
        to_face = mo.point_face_dist2(pts[b], verts[b], faces, face[b]).sqrt().numpy()
        err_face = max(err_face, float(np.abs(to_face - want).max()))
        s, t, off = (x.numpy() for x in mo.barycentric(closest[b], verts[b], faces, face[b]))
        assert min(s.min(), t.min()) >= -ON_FACE and (s + t).max() <= 1 + ON_FACE and off.max() <= ON_FACE, \
            (s.min(), t.min(), (s + t).max(), off.max())
        at = np.linalg.norm(closest[b].astype(np.float64) - pts[b].astype(np.float64), axis=1)
        assert np.abs(at - want).max() <= BAR, np.abs(at - want).max()
    print(f"PARITY pmdist {name} B={B} P={P} F={F}: max |kernel - fp64 oracle| = {err:.3e}, "
          f"max |fp32 restatement - fp64 oracle| = {err32:.3e}, max |fp64 dist to returned face - fp64 min| = {err_face:.3e} (bar {BAR:g})")
    assert err <= BAR and err_face <= BAR


def test_outputs_are_optional_and_not_differentiable(fsg, device):
    pts, verts, faces = _shape_case("odd_3x131x7")
    p, v, f = G(pts, device).requires_grad_(True), G(verts, device).requires_grad_(True), G(faces, device)
    full = fsg.functional.point_mesh_distance(p, v, f, return_face=True, return_closest=True)
    only = fsg.functional.point_mesh_distance(p, v, f)
    _, closest = fsg.functional.point_mesh_distance(p, v, f, return_closest=True)
    assert torch.is_tensor(only) and torch.equal(only, full[0]) and torch.equal(closest, full[2])
    assert not any(t.requires_grad for t in full)
    half = fsg.functional.point_mesh_distance(p.half(), v.double(), f.to(torch.int16))          # made fp32 / int32
    assert half.dtype == torch.float32 and torch.allclose(half, only, atol=2e-3)


@pytest.mark.parametrize("case", closed_form_cases() + degenerate_cases(), ids=lambda c: c[0])
def test_closed_forms_and_degenerate_faces_through_the_kernel(fsg, device, case):
    _, pts, verts, faces, want = case
    dist, face, closest = fsg.functional.point_mesh_distance(G(pts, device, torch.float32)[None], G(verts, device, torch.float32)[None],
                                                             G(faces, device), return_face=True, return_closest=True)
    dist, closest = N(dist[0]), N(closest[0])
    assert np.isfinite(dist).all() and np.isfinite(closest).all()
    np.testing.assert_allclose(dist, want, rtol=0, atol=BAR)
    np.testing.assert_allclose(np.linalg.norm(closest - pts, axis=1), want, rtol=0, atol=BAR)


def test_degenerate_faces_inside_a_mesh(fsg, device):
    """collapsed and collinear faces next to ordinary ones (a decoder early in training): finite, and equal to the oracle"""
    pts, verts, faces = _shape_case("pcae_2x2025x3872")
    verts, faces = verts.copy(), faces.copy()
    verts[0, 100:400] = verts[0, 100]                                     # 300 vertices collapse into one
    verts[1, :, 2] = 0
    verts[1, :, 1] = 0.5 * verts[1, :, 0]                                 # every vertex of mesh 1 on one line
    dist = N(fsg.functional.point_mesh_distance(G(pts, device), G(verts, device), G(faces, device)))
    assert np.isfinite(dist).all()
    for b in range(2):
        want = mo.point_mesh_dist2(pts[b], verts[b], faces)[0].sqrt().numpy()
        assert np.abs(dist[b] - want).max() <= BAR, (b, np.abs(dist[b] - want).max())


def test_shared_and_per_mesh_faces_agree_and_ties_take_the_lower_face(fsg, device):
    pts, verts, faces = _shape_case("pcae_2x2025x3872")
    p, v, f = G(pts, device), G(verts, device), G(faces, device)
    shared = fsg.functional.point_mesh_distance(p, v, f, return_face=True, return_closest=True)
    each = fsg.functional.point_mesh_distance(p, v, f[None].expand(2, -1, -1), return_face=True, return_closest=True)
    for a, b in zip(shared, each):
        assert torch.equal(a, b)
    twice = fsg.functional.point_mesh_distance(p, v, torch.cat([f, f]), return_face=True)       # every face once more, 3872 later
    assert torch.equal(twice[0], shared[0]) and torch.equal(twice[1], shared[1])


def test_face_indices_are_validated_once(fsg, device):
    pts, verts, faces = _shape_case("odd_3x131x7")
    bad = G(faces, device).clone()
    bad[3, 1] = verts.shape[1]
    with pytest.raises(ValueError, match="vertices"):
        fsg.functional.point_mesh_distance(G(pts, device), G(verts, device), bad)
    bad[3, 1] = 0                                                         # an in-place write: looked at again
    fsg.functional.point_mesh_distance(G(pts, device), G(verts, device), bad)
    n = len(fsg.functional._faces_checked)
    fsg.functional.point_mesh_distance(G(pts, device), G(verts, device), bad)
    assert len(fsg.functional._faces_checked) == n


def test_empty_inputs(fsg, device):
    verts, faces = torch.rand(2, 5, 3, device=device), torch.zeros(0, 3, dtype=torch.long, device=device)
    d, f, c = fsg.functional.point_mesh_distance(torch.rand(2, 4, 3, device=device), verts, faces, return_face=True, return_closest=True)
    assert d.shape == (2, 4) and torch.isnan(d).all() and (f == -1).all() and torch.isnan(c).all()
    d = fsg.functional.point_mesh_distance(torch.rand(2, 0, 3, device=device), verts, torch.tensor([[0, 1, 2]], device=device))
    assert d.shape == (2, 0)


def _assert_four(got, want, what):
    got, want = [float(x) for x in got], [float(x) for x in want]
    print(f"PARITY {what}: got {got}, oracle {want}")
    # mean, max and quantile move by at most the largest change of a distance, std by at most that again (fp32 sums are below it)
    np.testing.assert_allclose(got, want, rtol=0, atol=BAR)


def test_assd_and_batch_assd(fsg, device):
    from fissure_segmentation_amd import metrics
    vx, fx = mo.height_field_mesh(1311, 3, 20)
    vy, fy = mo.height_field_mesh(1312, 3, 24)
    per_item = []
    for b in range(3):
        got = metrics.assd((G(vx[b], device), G(fx, device)), (G(vy[b], device), G(fy, device)))
        assert all(t.dim() == 0 and t.is_cuda for t in got)
        _assert_four(got, mo.assd(vx[b], fx, vy[b], fy), f"assd item {b}")
        per_item.append(torch.stack(got))
    # open3d duck type (host arrays behind .vertices / .triangles) and array-likes
    duck = metrics.assd(SimpleNamespace(vertices=vx[0].astype(np.float64), triangles=fx), SimpleNamespace(vertices=vy[0].tolist(), triangles=fy))
    assert torch.equal(torch.stack(duck), per_item[0])
    batch = metrics.batch_assd(G(vx, device), G(fx, device)[None].expand(3, -1, -1), G(vy, device), G(fy, device)[None].expand(3, -1, -1))
    torch.testing.assert_close(torch.stack(batch), torch.stack(per_item).mean(0), rtol=1e-5, atol=1e-7)
    same = metrics.assd((G(vx[0], device), G(fx, device)), (G(vx[0], device), G(fx, device)))
    assert [float(x) for x in same] == [0.0, 0.0, 0.0, 0.0]
    d = metrics.point_surface_distance(vx[0], vy[0], fy)                   # array-likes in, one tensor out
    assert d.shape == (400,) and d.is_cuda


def test_pseudo_symmetric_point_to_mesh_distance(fsg, device):
    from fissure_segmentation_amd import metrics
    verts, faces = mo.height_field_mesh(1321, 1, 16)
    pts = mo.height_field_points(1322, 1, 3000)[0]
    v, f, n = G(verts[0], device), G(faces, device), 20000
    gen = torch.Generator(device=device)
    gen.manual_seed(77)
    samples, pick = metrics.sample_mesh_surface(v, f, n, gen)
    assert samples.shape == (n, 3) and int(pick.max()) < len(faces)
    on = fsg.functional.point_mesh_distance(samples[None], v[None], f)
    assert float(on.max()) <= 1e-5, float(on.max())
    gen.manual_seed(77)
    got = metrics.pseudo_symmetric_point_to_mesh_distance(G(pts, device), (v, f), n_samples=n, generator=gen)
    d_pm = mo.point_mesh_dist2(pts, verts[0], faces)[0].sqrt()
    d_mp = torch.cdist(samples.double().cpu(), torch.from_numpy(pts).double()).min(1).values
    _assert_four(got, mo.symmetric_point_distances(d_pm, d_mp), "pseudo_symmetric")
    # faces are drawn in proportion to their area: one face of three times the area of the other
    v2 = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [3, 1, 0]], device=device)
    f2 = torch.tensor([[0, 1, 2], [1, 3, 2]], device=device)               # areas 0.5 and 1.5
    n2 = 100000
    _, pick = metrics.sample_mesh_surface(v2, f2, n2, gen)
    count, sigma = int((pick == 1).sum()), (n2 * 0.75 * 0.25) ** 0.5
    assert abs(count - 0.75 * n2) <= 5 * sigma, (count, sigma)


def test_folding_net_mesh_goes_straight_in(fsg, device):
    """the path a user takes: decode a mesh, measure it against the input cloud and against another decoded mesh"""
    from fissure_segmentation_amd import metrics
    from fissure_segmentation_amd.models.folding_net import DGCNNFoldingNet
    net = fill_state_dict(DGCNNFoldingNet(k=8, n_embedding=64, shape_type="plane", n_input_points=1024, decode_mesh=True), 31)
    net = net.to(device).eval()
    x = G(cloud(1331, 2, 3, 1024), device)
    with torch.no_grad():
        verts = net(x).transpose(1, 2)                                    # (B, 1024, 3)
    faces = net.decoder.faces
    assert faces.shape == (2, 2 * 31 * 31, 3)
    dist = fsg.functional.point_mesh_distance(x.transpose(1, 2), verts, faces[0])
    want = mo.point_mesh_dist2(N(x[0].t()), N(verts[0]), N(faces[0]))[0].sqrt().numpy()
    scale = max(1.0, float(verts.abs().max()), float(x.abs().max()))      # the bar is stated for unit-scale coordinates
    assert np.abs(N(dist[0]) - want).max() <= BAR * scale
    assert torch.equal(dist, fsg.functional.point_mesh_distance(x.transpose(1, 2), verts, faces))
    out = metrics.batch_assd(verts, faces, verts.flip(0), faces)
    assert all(torch.isfinite(t) for t in out)
    out = metrics.pseudo_symmetric_point_to_mesh_distance(x[0].t(), (verts[0], faces[0]), n_samples=5000)
    assert all(torch.isfinite(t) for t in out)
