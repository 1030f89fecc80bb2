"""Generate tests/golden/dseg_ae_extend.npz by running the REAL reference's `random_extend_points`
(dseg_ae_regularization.py:115-138) on a seeded, duplicate-free cloud.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU.  Libraries that the
reference's module imports at its top and that `random_extend_points` never touches get inert placeholders where they are not
installed.  The cloud and the reference's three draws all come from ONE torch.manual_seed on the CPU generator, so the tests
replay them (tests/dseg_ae_oracle.py: golden_draws); stored are only the seed, the sizes, the reference's output, its mean and
standard deviation of the nearest distances, the fp64 oracle's output on the replayed draws and the largest difference between
the two -- the reference's own fp32 error.  No reference source text is written.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dseg_ae.py
"""
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

MAYBE_MISSING = ["SimpleITK", "pandas", "sklearn", "sklearn.cluster", "sklearn.decomposition", "matplotlib", "matplotlib.pyplot",
                 "matplotlib.colors", "matplotlib.cm", "mpl_toolkits", "mpl_toolkits.mplot3d", "mpl_toolkits.mplot3d.art3d",
                 "batchgenerators", "batchgenerators.transforms", "batchgenerators.transforms.abstract_transforms",
                 "batchgenerators.transforms.spatial_transforms", "batchgenerators.augmentations",
                 "batchgenerators.augmentations.utils", "skimage", "skimage.color", "skimage.measure", "skimage.morphology", "cv2",
                 "nibabel", "pykeops", "pykeops.torch", "tqdm", "seaborn", "imageio", "welford", "pycpd", "pyvista", "totalsegmentator",
                 "totalsegmentator.python_api", "lungmask", "torch_geometric", "wandb", "tikzplotlib", "scipy.spatial.transform"]


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import _Inert, import_reference
    import numpy as np
    import torch
    import dseg_ae_oracle as do
    from golden_util import GOLDEN_DIR
    import_reference()
    for name in MAYBE_MISSING:
        if name in sys.modules:
            continue
        try:
            importlib.import_module(name)
        except Exception:   # noqa: BLE001  (not installed, or not importable here: never touched by what runs below)
            m = _Inert(name)
            m.__path__ = []
            sys.modules[name] = m
    for _ in range(64):     # (anything else the import chain asks for that is not installed)
        try:
            r_dseg = importlib.import_module("dseg_ae_regularization")
            break
        except ModuleNotFoundError as e:
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                if ".".join(parts[:i]) not in sys.modules:
                    m = _Inert(".".join(parts[:i]))
                    m.__path__ = []
                    sys.modules[m.__name__] = m
    else:
        raise RuntimeError("the reference's dseg_ae_regularization still does not import after 64 placeholders")
    import utils.general_utils as r_gu

    torch.set_num_threads(8)
    n, target = do.GOLDEN_N, do.GOLDEN_TARGET
    torch.manual_seed(do.GOLDEN_SEED)
    points = torch.rand(1, n, 3)
    assert len(np.unique(points[0].numpy(), axis=0)) == n, "the cloud has duplicate points"
    ref = r_dseg.random_extend_points(points, target)
    assert ref.shape == (1, target, 3) and not torch.isnan(ref).any(), "the reference's output has NaN"
    dist = r_gu.knn(points.transpose(1, 2), 1, self_loop=False, return_dist=True)[1].sqrt()
    assert not torch.isnan(dist).any()

    p2, src, direction, z = do.golden_draws()
    assert torch.equal(p2, points)
    oracle, _, stats = do.extend(points[0].numpy(), [n], target, src.numpy(), direction.numpy(), z.numpy())
    err = float(np.abs(ref[0].numpy().astype(np.float64) - oracle).max())
    assert np.array_equal(ref[0, :n].numpy(), points[0].numpy()) and err < 1e-4, f"the replayed draws are not the reference's ({err})"
    path = os.path.join(GOLDEN_DIR, "dseg_ae_extend.npz")
    np.savez_compressed(path, seed=do.GOLDEN_SEED, n=n, target=target, ref_out=ref[0].numpy(),
                        ref_stats=np.array([dist.mean().item(), dist.std().item()], np.float64), oracle_out=oracle,
                        oracle_stats=stats[0], ref_error=err)
    print("wrote", path, os.path.getsize(path), "bytes; reference's error", err, "stats", stats[0], dist.mean().item(), dist.std().item())
    assert os.path.getsize(path) < 300_000


if __name__ == "__main__":
    main()
