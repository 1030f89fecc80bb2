"""Generate tests/golden/frontend_*.npz by running the REAL reference's image front end on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU with torch alone:
`data_processing.foerstner.foerstner_kpts`, `data_processing.point_features.mind`, `utils.image_utils.{smooth, nms}` and
`utils.general_utils.{kpts_to_grid, kpts_to_world, sample_patches_at_kpts}`.  The inputs are regenerated from seeds
(tests/frontend_oracle.py), only outputs are stored; no reference source text is written.  The volume seed is
reject-sampled until every keypoint decision of every configuration has a relative margin of at least MIN_MARGIN (as the
kNN fixtures are), so that fp32 rounding cannot change a keypoint list.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_frontend.py
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
MIN_MARGIN = 1e-3


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import _Inert, import_reference
    import numpy as np
    import torch
    import frontend_oracle as fo
    from golden_util import GOLDEN_DIR
    import_reference()
    for name in ["SimpleITK", "batchgenerators", "batchgenerators.transforms", "batchgenerators.transforms.abstract_transforms",
                 "batchgenerators.transforms.spatial_transforms", "skimage", "skimage.color", "cv2", "nibabel", "pandas",
                 "seaborn", "tqdm", "sklearn", "sklearn.model_selection"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                m = _Inert(name)
                m.__path__ = []
                sys.modules[name] = m
    from data_processing import foerstner as r_foerstner
    from data_processing.point_features import mind as r_mind
    from utils import general_utils as r_gu
    from utils import image_utils as r_iu

    torch.set_num_threads(8)
    mask = fo.box_mask()

    def min_margin(img):
        worst = float("inf")
        for sigma, d in fo.KPT_CONFIGS:
            dist = fo.distinctiveness(img.double(), sigma)
            worst = min(worst, float(fo.decision_margins(dist, d, 1e-8).min()))
        return worst

    seed = fo.GOLDEN_SEED
    while min(min_margin(fo.ct_volume(seed)), min_margin(fo.ct_volume(seed, constant_block=True))) < MIN_MARGIN:
        seed += 1
        print('trying seed', seed, flush=True)
        if seed > fo.GOLDEN_SEED + 60:
            raise SystemExit('no seed with the required margin')
    if seed != fo.GOLDEN_SEED:
        raise SystemExit(f"GOLDEN_SEED {fo.GOLDEN_SEED} has a margin below {MIN_MARGIN}; set it to {seed}")
    img, img_const = fo.ct_volume(seed), fo.ct_volume(seed, constant_block=True)
    e2e = fo.distinctiveness(fo.ct_volume(fo.E2E_SEED, fo.E2E_SHAPE).double(), 0.5)
    e2e_margin = float(fo.decision_margins(e2e, 5, 1e-8)[fo.erode_mask(fo.box_mask(fo.E2E_SHAPE))[0, 0]].min())
    if e2e_margin < MIN_MARGIN:
        raise SystemExit(f"E2E_SEED {fo.E2E_SEED} has a margin of {e2e_margin}, below {MIN_MARGIN}")

    out = dict(seed=seed, shape=np.array(fo.GOLDEN_SHAPE))
    for sigma in fo.DIST_SIGMAS:
        out[f"dist_s{sigma}"] = r_foerstner.distinctiveness(img, sigma).numpy()
        out[f"dist_const_s{sigma}"] = r_foerstner.distinctiveness(img_const, sigma).numpy()
    for sigma, d in fo.KPT_CONFIGS:
        out[f"kpts_s{sigma}_d{d}"] = r_foerstner.foerstner_kpts(img, mask, sigma=sigma, d=d).numpy()
        out[f"kpts_const_s{sigma}_d{d}"] = r_foerstner.foerstner_kpts(img_const, mask, sigma=sigma, d=d).numpy()
    out["smooth_s0.8"] = r_iu.smooth(img, 0.8).numpy()
    out["nms_d5"] = r_iu.nms(out_t := torch.from_numpy(out["dist_s0.5"]), 5).numpy()
    out["nms_d4"] = r_iu.nms(out_t, 4).numpy()
    path = os.path.join(GOLDEN_DIR, "frontend_foerstner.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: len(v) for k, v in out.items() if k.startswith("kpts")})

    for ssc, dil in fo.MIND_CONFIGS:
        path = os.path.join(GOLDEN_DIR, f"frontend_mind_{'ssc' if ssc else 'plain'}_d{dil}.npz")
        planes = list(fo.MIND_GOLDEN_PLANES)   # a fixed subset of z planes, both borders included, keeps the fixtures small
        np.savez_compressed(path, seed=seed, planes=np.array(planes),
                            mind=r_mind(img, dilation=dil, sigma=0.8, ssc=ssc).numpy()[:, :, planes])
        print("wrote", path, os.path.getsize(path), "bytes")

    out = dict(seed=seed)
    pts = fo.patch_points(seed + 1, 40)
    shape = torch.tensor(fo.GOLDEN_SHAPE)
    grid = r_gu.kpts_to_grid(pts, shape, align_corners=r_gu.ALIGN_CORNERS)
    out["grid"], out["world"] = grid.numpy(), r_gu.kpts_to_world(grid, shape, align_corners=r_gu.ALIGN_CORNERS).numpy()
    for ps in fo.PATCH_SIZES:
        out[f"patches_p{ps}"] = r_gu.sample_patches_at_kpts(img, grid, ps).numpy()
    path = os.path.join(GOLDEN_DIR, "frontend_points.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
