"""Generate tests/golden/seg_cnn_{net,patch}.npz by running the REAL reference's voxel CNN on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU: `models.seg_cnn.MobileNetASPP`
with the weights of tests/golden_util.fill_state_dict, its helpers `get_patch_starts`, `get_necessary_padding`,
`maybe_pad_img_patch`, `maybe_crop_after_padding` and `PatchBasedModule._get_gaussian`.  The inputs are regenerated from seeds
(tests/seg_cnn_oracle.py: `volume`), only seeds, settings and outputs are stored; no reference source text is written.

The training-mode forward is recorded with the ASPP's Dropout set to p = 0 on the reference's module (its mask is random and a
CPU stream cannot be replayed on the device); batch-statistics BatchNorm is what that fixture pins.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_seg_cnn.py
"""
import contextlib
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

WEIGHT_SEED, NUM_CLASSES = 11, 3
HELPER_CASES = [((40, 40, 40), 0.5, (16, 16, 16)), ((10, 20, 19), 0.5, (16, 16, 16)), ((33, 17, 64), 0.25, (16, 16, 32)),
                ((24, 16, 16), 0.5, (16, 16, 16)), ((21, 50, 7), 0.0, (8, 12, 16)), ((256, 256, 320), 0.5, (128, 128, 128))]
PAD_CASES = [((10, 16, 16), (16, 16, 16)), ((11, 13, 16), (16, 16, 16)), ((16, 16, 16), (16, 16, 16)), ((5, 16, 9), (8, 16, 16))]
GAUSS_PATCHES = [(9, 8, 12), (16, 16, 16)]
FORWARD_CASES = [("fwd16", 21, (2, 1, 16, 16, 16)), ("fwd8x12x16", 22, (1, 1, 8, 12, 16))]
PATCH_CASE = dict(seed=23, shape=(1, 1, 10, 20, 19), patch=(16, 16, 16), min_overlap=0.5)
TRAIN_CASE = dict(seed=24, shape=(2, 1, 16, 16, 16))
INPUT_SCALE = 3.0


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import import_reference
    import numpy as np
    import torch
    import seg_cnn_oracle as so
    from golden_util import GOLDEN_DIR, fill_state_dict

    import_reference()
    import models.seg_cnn as r

    torch.set_num_threads(8)

    def quiet(fn, *args, **kw):     # the reference prints every patch
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*args, **kw)

    net = fill_state_dict(r.MobileNetASPP(NUM_CLASSES, patch_size=PATCH_CASE["patch"]), WEIGHT_SEED).eval()
    sd = net.state_dict()
    out = dict(weight_seed=WEIGHT_SEED, num_classes=NUM_CLASSES, input_scale=INPUT_SCALE,
               keys=np.array(list(sd.keys())), shapes=np.array([json.dumps(list(v.shape)) for v in sd.values()]))
    helpers = dict(patch_starts=[dict(size=s, min_overlap=o, patch=p, starts=r.get_patch_starts(s, o, p)) for s, o, p in HELPER_CASES],
                   padding=[dict(size=s, patch=p, pad=r.get_necessary_padding(s, p),
                                 padded=list(r.maybe_pad_img_patch(torch.zeros(1, 1, *s), p).shape[2:])) for s, p in PAD_CASES])
    out["helpers_json"] = np.array(json.dumps(helpers))
    # pad -> crop gives the patch back, and where the crop starts (the front padding)
    x = torch.arange(11 * 13 * 16, dtype=torch.float32).view(1, 1, 11, 13, 16)
    padded = r.maybe_pad_img_patch(x, (16, 16, 16))
    assert torch.equal(r.maybe_crop_after_padding(padded, (11, 13, 16)), x)
    out["padded_11x13x16"] = padded[0, 0].numpy()
    for p in GAUSS_PATCHES:
        pm = r.PatchBasedModule(NUM_CLASSES)
        out["gauss_" + "x".join(map(str, p))] = pm._get_gaussian(p, "cpu", sigma_scale=1 / 4.)[0, 0].numpy().astype(np.float64)
    with torch.no_grad():
        for name, seed, shape in FORWARD_CASES:
            out[name + "_seed"], out[name + "_shape"] = seed, np.array(shape)
            out[name] = net(so.volume(seed, shape, INPUT_SCALE)).numpy()
    net.train()
    net.aspp.project[3].p = 0.0
    out["train_seed"], out["train_shape"] = TRAIN_CASE["seed"], np.array(TRAIN_CASE["shape"])
    out["train"] = net(so.volume(TRAIN_CASE["seed"], TRAIN_CASE["shape"], INPUT_SCALE)).detach().numpy()
    path = os.path.join(GOLDEN_DIR, "seg_cnn_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")

    net = fill_state_dict(r.MobileNetASPP(NUM_CLASSES, patch_size=PATCH_CASE["patch"]), WEIGHT_SEED).eval()
    img = so.volume(PATCH_CASE["seed"], PATCH_CASE["shape"], INPUT_SCALE)
    out = dict(weight_seed=WEIGHT_SEED, num_classes=NUM_CLASSES, input_scale=INPUT_SCALE, seed=PATCH_CASE["seed"],
               shape=np.array(PATCH_CASE["shape"]), patch=np.array(PATCH_CASE["patch"]), min_overlap=PATCH_CASE["min_overlap"])
    with torch.no_grad():
        out["gaussian"] = quiet(net.predict_all_patches, img, min_overlap=PATCH_CASE["min_overlap"], use_gaussian=True).numpy()
        out["uniform"] = quiet(net.predict_all_patches, img, min_overlap=PATCH_CASE["min_overlap"], use_gaussian=False).numpy()
    path = os.path.join(GOLDEN_DIR, "seg_cnn_patch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
