"""Generate tests/golden/tps_ref.npz by running the REAL reference's thin-plate-spline code on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU; the modules the reference
imports that are not installed are inert placeholders.  Recorded, outputs only (the inputs are regenerated from their seeds by
tests/tps_oracle.py and tests/kmeans_oracle.correspondence_inputs; no reference source text is written):

* shape_model.point_cloud_registration.TPS.fit (lambd = 0.1) and TPS.z of that fit at n = 5 and n = 257;
* thin_plate_dense on shape (36, 28, 20), step 4 -- a (9, 7, 5) lattice --, at 256 seeded voxels of the field;
* interpolate_displacements_tps on images (22, 30, 37) and (64, 64, 64);
* inverse_transformation_at_sampled_points(..., 'tps') on the first of those;
* shape_model.generate_corresponding_points.data_set_correspondences(mode='simple', interpolation_mode='tps') with the same
  stand-ins for open3d and pytorch3d as tools/make_golden_correspondences.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_tps.py
"""
import copy
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import _Inert, import_reference
    import numpy as np
    import torch
    from golden_util import GOLDEN_DIR
    import kmeans_oracle as ko
    import metrics_oracle as mo
    import tps_oracle as to
    from make_golden_correspondences import _Null
    import_reference()
    for name in ["SimpleITK", "batchgenerators", "batchgenerators.transforms", "batchgenerators.transforms.abstract_transforms",
                 "batchgenerators.transforms.spatial_transforms", "skimage", "skimage.color", "skimage.measure",
                 "skimage.morphology", "cv2", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "tqdm",
                 "pycpd", "pyamg", "nibabel", "pandas", "seaborn", "sklearn", "sklearn.decomposition", "sklearn.cluster",
                 "scipy.spatial.transform", "imageio", "pytorch3d.renderer", "pytorch3d.io", "pytorch3d.utils"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = _Inert(name)
                m.__path__ = []
                sys.modules[name] = m
    import shape_model.generate_corresponding_points as r_gcp
    import shape_model.point_cloud_registration as r_pcr

    torch.set_num_threads(8)
    t = torch.from_numpy
    out = {}
    with torch.no_grad():
        for n in to.GOLDEN_FIT:
            c, f, x = to.golden_fit_inputs(n)
            theta = r_pcr.TPS.fit(t(c), t(f), to.LAMBDA)
            out[f"fit{n}_theta"] = theta.numpy()
            out[f"fit{n}_z"] = r_pcr.TPS.z(t(x), t(c), theta).numpy()

        c, f, idx = to.golden_dense_inputs()
        field = r_pcr.thin_plate_dense(t(c)[None], t(f)[None], to.GOLDEN_DENSE_SHAPE, to.STEP, to.LAMBDA)
        out["dense_at_voxels"] = field.reshape(-1, 3)[idx].numpy()

        for shape in to.GOLDEN_IMG_SHAPES:
            e, v, q = to.golden_voxel_inputs(shape)
            out["interp_" + "_".join(map(str, shape))] = r_pcr.interpolate_displacements_tps(t(e)[None], t(v)[None], t(q)[None], shape)
        shape = to.GOLDEN_IMG_SHAPES[0]
        e, v, q = (a.astype(np.float64) for a in to.golden_voxel_inputs(shape))
        out["inverse"] = r_pcr.inverse_transformation_at_sampled_points(e, v, q, shape, 'tps')

    r_gcp.point_surface_distance = lambda query_points, trg_points, trg_tris: mo.point_mesh_dist2(
        torch.as_tensor(np.asarray(query_points)).double(), np.asarray(trg_points), np.asarray(trg_tris))[0].sqrt()
    r_gcp.pytorch3d.loss = type("loss", (), {"chamfer_distance": staticmethod(
        lambda x, y: (torch.tensor(ko.chamfer_pair(x.numpy(), y.numpy())), None))})
    r_gcp.plt = _Null()
    r_gcp.point_cloud_on_axis = r_gcp.trimesh_on_axis = _Null()
    r_gcp.tqdm_redirect = lambda it, **k: it
    inp = ko.correspondence_inputs()
    transforms = np.array(copy.deepcopy(inp["transforms"]), dtype=object)
    pcs, tr, fixed, labels, ev = r_gcp.data_set_correspondences(
        inp["fixed_pcs"], inp["meshes"], inp["moving_pcs"], transforms, inp["moved_pcs"], inp["displacements"],
        fixed_img_shape=to.GOLDEN_CORR_SHAPE, plot_dir=os.devnull, show=False, mode="simple", undo_affine_reg=True,
        interpolation_mode="tps")
    out["corr_pcs"], out["corr_fixed"], out["corr_labels"] = np.asarray(pcs), np.asarray(fixed), np.asarray(labels)
    for k, v in ev.items():
        out[f"corr_{k}"] = v.numpy()

    path = os.path.join(GOLDEN_DIR, "tps_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
