"""Generate tests/golden/dpsr_*.npz by running the REAL reference's DPSR front on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU: `models.divroc.DiVRoC`
(forward and both gradients), `models.dpsr_utils.point_rasterize` / `grid_interp`, `models.dpsr_net.DPSR` (forward and the
gradients to V and N at 16^3), the taps of `utils.image_utils.gaussian_kernel_1d`, and the PSR field of
`models.seg_logits_to_mesh.SoftMesh` -- captured by setting the instance attribute `psr_grid_to_mesh` to a function that keeps
its argument and stops the call, so no marching cubes (pytorch3d) is needed.  Those modules import a long chain at their top
(matplotlib, yaml, trimesh, plyfile, skimage, igl, open3d, pytorch3d ...) that these functions never touch: a fallback on
sys.meta_path answers any import that fails and was requested from a reference module with an inert stand-in.  The inputs are
regenerated from seeds (tests/dpsr_oracle.py), only outputs are stored; no reference source text is written.

The scale step of DPSR divides by |phi[0, 0, 0]|: every stored PSR case is first run unscaled and must have
|phi[0, 0, 0]| >= 0.1 max |phi|.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dpsr.py
"""
import importlib.abc
import importlib.machinery
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


class _Captured(Exception):
    pass


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import REF, _Inert, import_reference
    import numpy as np
    import torch
    import dpsr_oracle as do
    from golden_util import GOLDEN_DIR

    class Fallback(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        """last on sys.meta_path: reached only when no real module exists"""

        def find_spec(self, name, path=None, target=None):
            f = sys._getframe(1)
            while f is not None and "importlib" in f.f_code.co_filename:
                f = f.f_back
            if f is None or not os.path.abspath(f.f_code.co_filename).startswith(REF + os.sep):
                return None
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

        def create_module(self, spec):
            m = _Inert(spec.name)
            m.__path__ = []
            return m

        def exec_module(self, module):
            print("  stand-in for", module.__name__)

    import_reference()
    sys.meta_path.append(Fallback())
    from models.divroc import DiVRoC
    from models.dpsr_net import DPSR
    from models.dpsr_utils import grid_interp, point_rasterize
    from models.seg_logits_to_mesh import SoftMesh
    from utils.image_utils import gaussian_kernel_1d

    torch.set_num_threads(8)

    def save(name, **arrs):
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **{k: np.ascontiguousarray(v.detach().numpy()) for k, v in arrs.items()})
        print("wrote", path, os.path.getsize(path), "bytes")

    def leaf(t):
        return t.clone().requires_grad_(True)

    # ---- DiVRoC (divroc.py:24-61): coords in [-1.2, 1.2], a non-cubic grid
    c = do.cloud_case(do.SEEDS["torch", 3])
    B, C, N = c["values"].shape
    v, x = leaf(c["values"]), leaf(c["coords"])
    out = DiVRoC.apply(v.view(B, C, N, 1, 1), x.view(B, N, 1, 1, 3), (B, C, *do.GRID))
    (out * c["g_grid"]).sum().backward()
    save("dpsr_divroc", out=out, grad_values=v.grad, grad_coords=x.grad)

    # ---- point_rasterize / grid_interp (dpsr_utils.py:156-287): points in [0, 1], and node points
    c = do.cloud_case(do.SEEDS["sap", 3], lo=0.0, hi=1.0)
    v, x = leaf(c["values"]), leaf(c["coords"])
    ras = point_rasterize(x, v.transpose(1, 2), do.GRID)
    (ras * c["g_grid"]).sum().backward()
    out = dict(raster=ras, raster_grad_vals=v.grad, raster_grad_pts=x.grad)
    g, x = leaf(c["grid"]), leaf(c["coords"])
    it = grid_interp(g.permute(0, 2, 3, 4, 1), x)                                   # (B, N, C)
    (it.transpose(1, 2) * c["g_pts"]).sum().backward()
    out.update(interp=it, interp_grad_grid=g.grad, interp_grad_pts=x.grad)
    nodes = do.node_coords("sap")
    nv = do.cloud_case(3, B=1, N=nodes.shape[1])
    with torch.no_grad():
        out["raster_nodes"] = point_rasterize(nodes, nv["values"].transpose(1, 2), do.GRID)
        out["interp_nodes"] = grid_interp(nv["grid"].permute(0, 2, 3, 4, 1), nodes)
    save("dpsr_sap", **out)

    # ---- DPSR (dpsr_net.py:32-104) at 16^3, sig 2, on a sphere; Gaussian-derivative taps
    s = do.sphere_case()
    with torch.no_grad():
        raw = DPSR(do.RES, do.SIG, scale=False, shift=True)(s["V"], s["N"])
    ratio = raw[:, 0, 0, 0].abs() / raw.flatten(1).abs().max(1).values
    print("DPSR |phi0| / max |phi| per item:", ratio.tolist())
    assert bool((ratio >= 0.1).all()), "ill-conditioned scale step"
    V, Nn = leaf(s["V"]), leaf(s["N"])
    phi = DPSR(do.RES, do.SIG)(V, Nn)
    (phi * s["g_phi"]).sum().backward()
    taps = {f"taps_s{str(sig).replace('.', 'p')}_o{order}_t{str(tr).replace('.', 'p')}": gaussian_kernel_1d(sig, order, tr)
            for sig, order, tr in ((10, 1, 1.5), (2.0, 1, 1.5), (2.0, 0, 4.0), (1.5, 2, 4.0))}
    save("dpsr_psr", phi=phi, grad_V=V.grad, grad_N=Nn.grad, **taps)

    # ---- SoftMesh (seg_logits_to_mesh.py:57-116): the PSR field, captured before marching cubes
    m = do.softmesh_case()

    def field(scale, logits):
        sm = SoftMesh(do.SMOOTH_SIGMA, do.RES, do.SIG, dpsr_scale=scale, dpsr_shift=True)
        got = []

        def capture(grid):
            got.append(grid)
            raise _Captured

        sm.psr_grid_to_mesh = capture
        try:
            sm(logits, m["coords"])
        except _Captured:
            pass
        return got[0]

    with torch.no_grad():
        raw = field(False, m["logits"])
    ratio = raw[:, 0, 0, 0].abs() / raw.flatten(1).abs().max(1).values
    print("SoftMesh |phi0| / max |phi| per grid:", ratio.tolist())
    assert bool((ratio >= 0.1).all()), "ill-conditioned scale step"
    lg = leaf(m["logits"])
    f = field(True, lg)
    (f * m["g_field"]).sum().backward()
    save("dpsr_softmesh", field=f, grad_logits=lg.grad)


if __name__ == "__main__":
    main()
