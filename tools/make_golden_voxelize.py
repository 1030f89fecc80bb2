"""Generate tests/golden/voxelize_ref.npz by running the REAL reference on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU with torch alone; the
modules the reference imports that are not installed are inert placeholders.  Recorded, outputs only (the inputs are
regenerated from seeds by tests/voxelize_oracle.py; no reference source text is written):

* utils.general_utils.mask_to_points and points_to_label_map on voxelize_oracle.util_inputs();
* data_processing.surface_fitting_optimization.mesh2labelmap_dist on the three sheets at thresholds 1.0 and 1.5, with and
  without the random mask -- its `point_surface_distance` (open3d, not available) bound to the fp64 oracle
  metrics_oracle.point_mesh_dist2, so what is pinned is the reference's own argmin / threshold / mask / scatter;
* data_processing.surface_fitting.o3d_mesh_to_labelmap on duck meshes whose `sample_points_uniformly` returns the seeded
  samples of voxelize_oracle.sample_surface (in x, y, z), WITHOUT the samples that have a negative coordinate: the
  reference truncates those into cell 0 or lets the negative index wrap to the far side of the volume, which the package
  deliberately does not reproduce.

Each of the last two is skipped, and `have_dist` / `have_o3d` say so, if its module does not import this way.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_voxelize.py
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import _Inert, import_reference
    import numpy as np
    import torch
    from golden_util import GOLDEN_DIR
    import metrics_oracle as mo
    import voxelize_oracle as vo
    import_reference()
    for name in ["SimpleITK", "batchgenerators", "batchgenerators.transforms", "batchgenerators.transforms.abstract_transforms",
                 "batchgenerators.transforms.spatial_transforms", "skimage", "skimage.color", "skimage.measure", "cv2",
                 "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "tqdm", "pycpd", "pyamg", "nibabel",
                 "pandas", "seaborn", "sklearn", "sklearn.decomposition", "scipy.spatial.transform"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = _Inert(name)
                m.__path__ = []
                sys.modules[name] = m
    import utils.general_utils as r_gu

    torch.set_num_threads(8)
    out = {}
    mask, pts, labels = vo.util_inputs()
    out["mask_to_points"] = r_gu.mask_to_points(torch.from_numpy(mask), vo.UTIL_SPACING_XYZ).numpy()
    lm, idx = r_gu.points_to_label_map(torch.from_numpy(pts), torch.from_numpy(labels), vo.UTIL_SHAPE, vo.UTIL_SPACING_XYZ)
    out["points_label_map"], out["points_index"] = lm.numpy(), idx.numpy()

    meshes = vo.sheets()
    spacing_xyz = vo.SPACING[::-1]
    why = {}
    try:
        import data_processing.surface_fitting_optimization as r_sfo
        r_sfo.point_surface_distance = lambda q, v, f: mo.point_mesh_dist2(q.double(), v, f)[0].sqrt()
        tm = [(torch.from_numpy(v), torch.from_numpy(f)) for v, f in meshes]
        rmask = torch.from_numpy(vo.random_mask())
        for thr in (1.0, 1.5):
            for tag, m in (("", None), ("_mask", rmask)):
                out[f"dist_{thr}{tag}"] = r_sfo.mesh2labelmap_dist(tm, vo.SHAPE, spacing_xyz, thr, m).numpy().astype(np.uint8)
    except Exception as e:   # noqa: BLE001
        why["dist"] = f"{type(e).__name__}: {e}"
    out["have_dist"] = "dist" not in why

    try:
        import data_processing.surface_fitting as r_sf

        class Duck:
            def __init__(self, verts, faces, seed):
                self.vertices, self.triangles, self.seed = verts[:, ::-1], faces, seed
                self.volume_order = (verts, faces)

            def sample_points_uniformly(self, number_of_points):
                p = vo.sample_surface(*self.volume_order, number_of_points, self.seed)
                p = p[(p >= 0).all(1)]
                return type("Cloud", (), {"points": np.ascontiguousarray(p[:, ::-1])})()
        ducks = [Duck(v, f, vo.SAMPLE_SEED + m) for m, (v, f) in enumerate(meshes)]
        out["o3d_all"] = r_sf.o3d_mesh_to_labelmap(ducks, vo.SHAPE, spacing_xyz, n_samples=vo.N_SAMPLES).numpy().astype(np.uint8)
    except Exception as e:   # noqa: BLE001
        why["o3d"] = f"{type(e).__name__}: {e}"
    out["have_o3d"] = "o3d" not in why

    for k, v in why.items():
        print("NOT recorded:", k, "--", v)
    path = os.path.join(GOLDEN_DIR, "voxelize_ref.npz")
    np.savez_compressed(path, util_seed=vo.UTIL_SEED, sample_seed=vo.SAMPLE_SEED, n_samples=vo.N_SAMPLES, **out)
    print("wrote", path, os.path.getsize(path), "bytes:", sorted(out))


if __name__ == "__main__":
    main()
