"""Generate tests/golden/correspondences_ref.npz by running the REAL reference's data_set_correspondences on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU; the modules the reference
imports that are not installed are inert placeholders.  Recorded, outputs only (the inputs are regenerated from the seed by
tests/kmeans_oracle.correspondence_inputs; no reference source text is written):

* shape_model.generate_corresponding_points.data_set_correspondences in mode 'simple' with and without `undo_affine_reg`, and
  in mode 'kmeans' under np.random.seed(KMEANS_SEED) -- there also sklearn's centroids (the returned corresponding_fixed_pc),
  so that everything after the clustering can be pinned without sklearn's random stream;
* with its `point_surface_distance` (open3d, not available) bound to the fp64 oracle metrics_oracle.point_mesh_dist2(..).sqrt(),
  `pytorch3d.loss.chamfer_distance` to the numpy restatement kmeans_oracle.chamfer_pair, and the plotting calls to no-ops; the
  kNN interpolation, the affine undo, the clustering call, the statistics and the assembly of the outputs are the reference's.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_correspondences.py
"""
import copy
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
KMEANS_SEED = 7


class _Null:
    """stands where matplotlib would draw: every attribute and every call gives the same nothing"""

    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import _Inert, import_reference
    import numpy as np
    import torch
    from golden_util import GOLDEN_DIR
    import kmeans_oracle as ko
    import metrics_oracle as mo
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
    import sklearn

    torch.set_num_threads(8)
    r_gcp.point_surface_distance = lambda query_points, trg_points, trg_tris: mo.point_mesh_dist2(
        torch.as_tensor(np.asarray(query_points)).double(), np.asarray(trg_points), np.asarray(trg_tris))[0].sqrt()
    r_gcp.pytorch3d.loss = type("loss", (), {"chamfer_distance": staticmethod(
        lambda x, y: (torch.tensor(ko.chamfer_pair(x.numpy(), y.numpy())), None))})
    r_gcp.plt = _Null()
    r_gcp.point_cloud_on_axis = r_gcp.trimesh_on_axis = _Null()
    r_gcp.tqdm_redirect = lambda it, **k: it

    def run(tag, out, **kw):
        inp = ko.correspondence_inputs()
        transforms = np.array(copy.deepcopy(inp["transforms"]), dtype=object)
        pcs, tr, fixed, labels, ev = r_gcp.data_set_correspondences(
            inp["fixed_pcs"], inp["meshes"], inp["moving_pcs"], transforms, inp["moved_pcs"], inp["displacements"],
            fixed_img_shape=(256, 256, 256), plot_dir=os.devnull, show=False, **kw)
        out[f"{tag}_pcs"], out[f"{tag}_fixed"], out[f"{tag}_labels"] = np.asarray(pcs), np.asarray(fixed), np.asarray(labels)
        out[f"{tag}_is_applied"] = np.array([bool(t["is_applied"]) for t in tr])
        for k, v in ev.items():
            out[f"{tag}_{k}"] = v.numpy()

    out = {}
    run("simple_undo", out, mode="simple", undo_affine_reg=True)
    run("simple_keep", out, mode="simple", undo_affine_reg=False)
    np.random.seed(KMEANS_SEED)
    run("kmeans_undo", out, mode="kmeans", undo_affine_reg=True)
    path = os.path.join(GOLDEN_DIR, "correspondences_ref.npz")
    np.savez_compressed(path, seed=ko.CORR_SEED, kmeans_seed=KMEANS_SEED, sklearn_version=sklearn.__version__, **out)
    print("wrote", path, os.path.getsize(path), "bytes:", sorted(out))


if __name__ == "__main__":
    main()
