"""Generate tests/golden/metrics_torch.npz by running the REAL reference's metrics.py on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU with torch alone.  The
inert open3d placeholder is enough to import the module; everything behind open3d (point_surface_distance, assd, batch_assd,
pseudo_symmetric_point_to_mesh_distance) cannot run and is not pinned here -- tests/metrics_oracle.py says what pins the
distance itself.  Recorded: `_symmetric_point_distances`, `batch_dice`, `binary_recall`, `binary_precision`.  The inputs are
regenerated from seeds (metrics_oracle.summary_inputs / label_inputs), only outputs are stored; no reference source text is
written.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_metrics.py
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
    from metrics_oracle import LABEL_N, LABEL_SEED, SUMMARY_SEED, label_inputs, summary_inputs
    import_reference()
    for name in ["SimpleITK", "batchgenerators", "batchgenerators.transforms", "batchgenerators.transforms.abstract_transforms",
                 "batchgenerators.transforms.spatial_transforms", "skimage", "skimage.color", "cv2"]:
        if name not in sys.modules:
            m = _Inert(name)
            m.__path__ = []
            sys.modules[name] = m
    import metrics as r_metrics

    torch.set_num_threads(8)
    d1, d2 = (torch.from_numpy(a) for a in summary_inputs())
    mean, std, hd, hd95 = r_metrics._symmetric_point_distances(d1, d2)
    pred, targ = (torch.from_numpy(a) for a in label_inputs())
    path = os.path.join(GOLDEN_DIR, "metrics_torch.npz")
    np.savez_compressed(path, summary_seed=SUMMARY_SEED, label_seed=LABEL_SEED, n_labels=LABEL_N,
                        symmetric=np.array([mean.item(), std.item(), hd.item(), hd95.item()], dtype=np.float64),
                        dice=r_metrics.batch_dice(pred, targ, LABEL_N).numpy(), recall=r_metrics.binary_recall(pred, targ).numpy(),
                        precision=r_metrics.binary_precision(pred, targ).numpy())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
