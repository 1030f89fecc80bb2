"""CPU tests of the DPSR front (csrc/grid_points.hip, functional.splat_to_grid / sample_grid / psr_spectral_solve, models/divroc.py,
dpsr_utils.py, dpsr_net.py, seg_logits_to_mesh.py, utils/image_utils.gaussian_differentiation):

* the torch oracle of tests/dpsr_oracle.py against every fixture the real reference produced (tests/golden/dpsr_*.npz).  The
  reference ran in fp32, so the bar is the oracle's own fp32-vs-fp64 difference: |reference - oracle64| <= max(4 |oracle32 -
  oracle64|, 8 * 2^-24 * magnitude), the bar the GPU tests then hold the kernels to;
* the new symbols are declared, exported and bound; host-side argument validation of the C ABI and of the Python layers;
* the Gaussian-derivative taps (built without scipy) against the reference's."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dpsr_oracle as do
from conftest import ROOT
from golden_util import load

NEW_SYMBOLS = ("fsg_grid_corners_f32", "fsg_grid_splat_workspace_bytes", "fsg_grid_splat_sorted_f32", "fsg_grid_sample_f32",
               "fsg_psr_spectral_f32")


def _check(label, got, want64, want32):
    ok, msg = do.bar("DPSR_GOLDEN", label, torch.from_numpy(np.asarray(got)), want64.detach(), want32.detach())
    assert ok, msg


def _both(fn):
    """run fn(dtype) -> tuple of tensors in fp64 and fp32"""
    return fn(torch.float64), fn(torch.float32)


def test_oracle_matches_divroc_golden():
    g, c = load("dpsr_divroc"), do.cloud_case(do.SEEDS["torch", 3])

    def run(dt):
        v, x = do.leaf(c["values"], dt), do.leaf(c["coords"], dt)
        out = do.splat(v, x, do.GRID, "torch")
        gv, gx = torch.autograd.grad((out * c["g_grid"].to(dt)).sum(), (v, x))
        return out, gv, gx
    o64, o32 = _both(run)
    assert bool(do.far_from_planes(c["coords"], do.GRID, "torch").all())
    for name, a, b in zip(("out", "grad_values", "grad_coords"), o64, o32):
        _check("divroc " + name, g[name], a, b)
    assert float(np.abs(g["out"]).max()) > 0.1


def test_oracle_matches_rasterize_and_interp_golden():
    g, c = load("dpsr_sap"), do.cloud_case(do.SEEDS["sap", 3], lo=0.0, hi=1.0)
    assert bool(do.far_from_planes(c["coords"], do.GRID, "sap").all())

    def ras(dt):
        v, x = do.leaf(c["values"], dt), do.leaf(c["coords"], dt)
        out = do.splat(v, x, do.GRID, "sap")
        return (out,) + torch.autograd.grad((out * c["g_grid"].to(dt)).sum(), (v, x))

    def interp(dt):
        gr, x = do.leaf(c["grid"], dt), do.leaf(c["coords"], dt)
        out = do.sample(gr, x, "sap")
        return (out.transpose(1, 2),) + torch.autograd.grad((out * c["g_pts"].to(dt)).sum(), (gr, x))
    for names, (o64, o32) in ((("raster", "raster_grad_vals", "raster_grad_pts"), _both(ras)),
                              (("interp", "interp_grad_grid", "interp_grad_pts"), _both(interp))):
        for name, a, b in zip(names, o64, o32):
            _check("sap " + name, g[name], a, b)


def test_oracle_matches_node_point_golden():
    """points on nodes, at 0 and at 1: the fp32 index rules decide the voxel"""
    g = load("dpsr_sap")
    nodes = do.node_coords("sap")
    nv = do.cloud_case(3, B=1, N=nodes.shape[1])
    r64, r32 = _both(lambda dt: (do.splat(nv["values"].to(dt), nodes.to(dt), do.GRID, "sap"),
                                 do.sample(nv["grid"].to(dt), nodes.to(dt), "sap").transpose(1, 2)))
    _check("sap raster_nodes", g["raster_nodes"], r64[0], r32[0])
    _check("sap interp_nodes", g["interp_nodes"], r64[1], r32[1])


def test_oracle_matches_dpsr_golden():
    g, s = load("dpsr_psr"), do.sphere_case()

    def run(dt):
        V, N = do.leaf(s["V"], dt), do.leaf(s["N"], dt)
        phi = do.dpsr(V, N)
        return (phi,) + torch.autograd.grad((phi * s["g_phi"].to(dt)).sum(), (V, N))
    o64, o32 = _both(run)
    raw = do.dpsr(s["V"].double(), s["N"].double(), prescale=True)
    assert bool((raw[:, 0, 0, 0].abs() >= 0.1 * raw.flatten(1).abs().max(1).values).all())
    for name, a, b in zip(("phi", "grad_V", "grad_N"), o64, o32):
        _check("dpsr " + name, g[name], a, b)


def test_oracle_matches_softmesh_golden():
    g, m = load("dpsr_softmesh"), do.softmesh_case()

    def run(dt):
        lg = do.leaf(m["logits"], dt)
        f = do.softmesh_field(lg, m["coords"].to(dt))
        return f, torch.autograd.grad((f * m["g_field"].to(dt)).sum(), lg)[0]
    o64, o32 = _both(run)
    _check("softmesh field", g["field"], o64[0], o32[0])
    _check("softmesh grad_logits", g["grad_logits"], o64[1], o32[1])


@pytest.mark.parametrize("sigma,order,truncate", [(10, 1, 1.5), (2.0, 1, 1.5), (2.0, 0, 4.0), (1.5, 2, 4.0)])
def test_gaussian_derivative_taps(sigma, order, truncate):
    """the taps are built in fp64 and rounded once, like scipy's: equal to the reference's to the last bit or the one before"""
    from fissure_segmentation_amd.utils.image_utils import gaussian_derivative_taps
    key = f"taps_s{str(sigma).replace('.', 'p')}_o{order}_t{str(truncate).replace('.', 'p')}"
    want = torch.from_numpy(load("dpsr_psr")[key])
    got = gaussian_derivative_taps(sigma, order, truncate)
    assert got.dtype == torch.float32 and got.shape == want.shape == (2 * int(truncate * sigma + 0.5) + 1,)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 2.0 ** -23 * scale
    assert float((got.double() - do.derivative_taps(sigma, order, truncate)).abs().max()) <= 2.0 ** -23 * scale


def test_gaussian_differentiation_is_the_one_axis_filter():
    from fissure_segmentation_amd.utils.image_utils import gaussian_differentiation
    img = torch.randn(2, 3, 6, 7, 9, generator=torch.Generator().manual_seed(0))
    for dim in (0, 1, 2):
        got = gaussian_differentiation(img, 2.0, order=1, dim=dim, padding_mode='constant', truncate=1.5)
        want = do._filter_axis(img.double(), do.derivative_taps(2.0, 1, 1.5), dim)
        assert got.shape == img.shape and float((got.double() - want).abs().max()) < 1e-5
    params = list(inspect.signature(gaussian_differentiation).parameters.values())
    assert [(p.name, p.default) for p in params[3:]] == [("dim", inspect.Parameter.empty), ("padding_mode", "replicate"),
                                                        ("truncate", 4.0)]


def test_symbols_declared_bound_and_exported():
    from fissure_segmentation_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsg_hip.h")).read()
    declared = set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "grid_points.hip" in open(os.path.join(ROOT, "fissure-segmentation_amd", "csrc", "Makefile")).read()
    assert "#define FSG_GRID_TORCH 0" in header and "#define FSG_GRID_SAP 1" in header
    assert (_lib.GRID_TORCH, _lib.GRID_SAP) == (0, 1)
    assert _lib.lib.fsg_grid_splat_workspace_bytes(2, 3, 50) == 2 * 3 * 8 * 50 * 4
    assert _lib.lib.fsg_grid_splat_workspace_bytes(2, 3, 0) == 0


def test_bad_arguments_are_reported_before_launch():
    """validation is on the host and comes first, so it is testable without a GPU (8 stands for a non-NULL pointer)"""
    from fissure_segmentation_amd import _lib
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_grid_corners_f32", None, 1, 4, 8, 8, 8, 0, 8, 8, None)
    with pytest.raises(RuntimeError, match="bad mode"):
        _lib.call("fsg_grid_corners_f32", 8, 1, 4, 8, 8, 8, 2, 8, 8, None)
    for B, N, D, H, W, mode in ((0, 4, 8, 8, 8, 0), (70000, 4, 8, 8, 8, 0), (1, 0, 8, 8, 8, 0), (1, 4, 0, 8, 8, 0),
                                (1, 4, 2048, 1024, 1024, 0), (1, 4, 1, 8, 8, 1), (1, (1 << 27) + 1, 8, 8, 8, 0)):
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_grid_corners_f32", 8, B, N, D, H, W, mode, 8, 8, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_grid_splat_sorted_f32", 8, 8, None, 8, 1, 1, 4, 8, 8, 8, 8, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("fsg_grid_splat_sorted_f32", 8, 8, 8, 8, 1, 0, 4, 8, 8, 8, 8, 8, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace of 127 bytes"):
        _lib.call("fsg_grid_splat_sorted_f32", 8, 8, 8, 8, 1, 1, 4, 8, 8, 8, 8, 8, 127, None)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("fsg_grid_splat_sorted_f32", 8, 8, 8, 8, 1, 1, 4, 8, 8, 8, 8, 6, 128, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_grid_sample_f32", 8, 8, None, 1, 1, 4, 8, 8, 8, 0, None, None, None)
    with pytest.raises(RuntimeError, match="come together"):
        _lib.call("fsg_grid_sample_f32", 8, 8, 8, 1, 1, 4, 8, 8, 8, 0, 8, None, None)
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("fsg_grid_sample_f32", 8, 8, None, 1, 1, 4, 8, 1, 8, 1, 8, None, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        _lib.call("fsg_psr_spectral_f32", 8, 1, 8, 8, 8, 2.0, 0, 8, None)            # in == out
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("fsg_psr_spectral_f32", 8, 1, 8, 0, 8, 2.0, 0, 16, None)
    for sig, adj in ((-1.0, 0), (2.0, 2)):
        with pytest.raises(RuntimeError, match="bad sig"):
            _lib.call("fsg_psr_spectral_f32", 8, 1, 8, 8, 8, sig, adj, 16, None)


def test_python_layers_validate_before_touching_the_device():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.models.divroc import DiVRoC
    from fissure_segmentation_amd.models.dpsr_utils import grid_interp, point_rasterize
    v, x, grid = torch.zeros(2, 3, 5), torch.zeros(2, 5, 3), torch.zeros(2, 3, 4, 5, 6)
    for mode in ("nearest", 0, None):
        with pytest.raises(ValueError, match="mode"):
            F_hip.splat_to_grid(v, x, (4, 5, 6), mode)
    for size in ((4, 5), (4, 5, 0), 7, (1, 5, 6)):
        with pytest.raises(ValueError, match="grid size"):
            F_hip.splat_to_grid(v, x, size, "sap")
    with pytest.raises(ValueError, match="number of points"):
        F_hip.splat_to_grid(v, torch.zeros(2, 6, 3), (4, 5, 6), "torch")
    for bad_x in (torch.zeros(2, 5, 2), torch.zeros(3, 5, 3), torch.zeros(2, 5)):
        with pytest.raises(ValueError, match="coords"):
            F_hip.splat_to_grid(v, bad_x, (4, 5, 6), "torch")
        with pytest.raises(ValueError, match="coords"):
            F_hip.sample_grid(grid, bad_x, "torch")
    with pytest.raises(ValueError, match="5 dimensions"):
        F_hip.sample_grid(grid[0], x, "torch")
    with pytest.raises(TypeError, match="floating-point"):
        F_hip.splat_to_grid(v.long(), x, (4, 5, 6), "torch")
    with pytest.raises(TypeError, match="floating-point"):
        F_hip.sample_grid(grid, x.int(), "sap")
    with pytest.raises(TypeError, match="complex64"):
        F_hip.psr_spectral_solve(torch.zeros(1, 3, 8, 8, 5), (8, 8, 8), 2.0)
    with pytest.raises(ValueError, match="expected normal_field_hat"):
        F_hip.psr_spectral_solve(torch.zeros(1, 3, 8, 8, 4, dtype=torch.complex64), (8, 8, 8), 2.0)
    with pytest.raises(ValueError, match="res"):
        F_hip.psr_spectral_solve(torch.zeros(1, 3, 8, 8, 5, dtype=torch.complex64), (8, 8), 2.0)
    with pytest.raises(ValueError, match="sig"):
        F_hip.psr_spectral_solve(torch.zeros(1, 3, 8, 8, 5, dtype=torch.complex64), (8, 8, 8), -1)
    with pytest.raises(ValueError, match="feature_values"):
        DiVRoC.apply(v, x.view(2, 5, 1, 1, 3), (2, 3, 4, 5, 6))
    with pytest.raises(ValueError, match="shape must be"):
        DiVRoC.apply(v.view(2, 3, 5, 1, 1), x.view(2, 5, 1, 1, 3), (2, 4, 4, 5, 6))
    with pytest.raises(NotImplementedError, match="3-D"):
        point_rasterize(torch.zeros(2, 5, 2), torch.zeros(2, 5, 1), (4, 4))
    with pytest.raises(NotImplementedError, match="3-D"):
        grid_interp(torch.zeros(2, 4, 4, 1), torch.zeros(2, 5, 2))
    # valid arguments on the CPU: refused, never computed by a fallback
    for fn in (lambda: F_hip.splat_to_grid(v, x, (4, 5, 6), "torch"), lambda: F_hip.sample_grid(grid, x, "SAP"),
               lambda: F_hip.psr_spectral_solve(torch.zeros(1, 3, 8, 8, 5, dtype=torch.complex64), (8, 8, 8), 2.0),
               lambda: point_rasterize(x, v.transpose(1, 2), (4, 5, 6))):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn()


def test_modules_keep_the_reference_names():
    from fissure_segmentation_amd.losses.access_losses import get_loss_fn  # noqa: F401  (the 'dpsr' routing is untouched)
    from fissure_segmentation_amd.models.dpsr_net import DPSR
    from fissure_segmentation_amd.models.dpsr_utils import fftfreqs, spec_gaussian_filter
    from fissure_segmentation_amd.models.seg_logits_to_mesh import SoftMesh
    sig = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]   # noqa: E731
    assert sig(DPSR.__init__) == [("res", inspect.Parameter.empty), ("sig", 10), ("scale", True), ("shift", True)]
    assert sig(SoftMesh.__init__) == [("smoothing_sigma", 10), ("dpsr_res", (128, 128, 128)), ("dpsr_sigma", 10),
                                      ("dpsr_scale", True), ("dpsr_shift", True), ("exclude_background", True)]
    d = DPSR((8, 10, 12), sig=3)
    assert list(d.state_dict()) == ["G"] and d.G.shape == (8, 10, 7, 1, 1) and d.G.dtype == torch.float32
    assert fftfreqs((8, 10, 12)).shape == (8, 10, 7, 3) and fftfreqs((8, 10, 12), exact=False).shape == (8, 10, 6, 3)
    assert torch.equal(fftfreqs((4, 4, 5))[:, 0, 0, 0], torch.tensor([0., 1., -2., -1.]))
    assert torch.equal(fftfreqs((4, 5, 5))[0, :, 0, 1], torch.tensor([0., 1., 2., -2., -1.]))
    f = do.freqs((8, 10, 12), torch.float64, "cpu")
    want = torch.exp(-0.5 * (3 * 2 * f.pow(2).sum(-1).sqrt() / 8) ** 2)
    assert torch.equal(spec_gaussian_filter((8, 10, 12), 3)[..., 0, 0], want)
    sm = SoftMesh(2, (16, 16, 16), 2)
    assert list(sm.state_dict()) == ["dpsr.G"]
    with pytest.raises(NotImplementedError, match="marching cubes"):
        sm(torch.zeros(1, 3, 4), torch.zeros(1, 3, 4))
    with pytest.raises(NotImplementedError, match="3-D"):
        DPSR((16, 16))
