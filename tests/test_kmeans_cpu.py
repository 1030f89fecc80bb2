"""CPU tests of the k-means port: the checkers themselves (tests/kmeans_oracle.py -- the bit-exact restatement of csrc/kmeans.hip
against the fp64 Lloyd and scipy's kmeans2), the properties the kernel's design rests on (order-independent fixed-point sums),
the real-reference fixture tests/golden/correspondences_ref.npz, and every refusal that happens before a launch."""
import os
import warnings

import numpy as np
import pytest
import torch

import kmeans_oracle as ko
from golden_util import GOLDEN_DIR

SIZES = {"12x37": (12, 37, 5), "20x256": (20, 256, 5)}   # instances, points per instance = K, seed


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, (I, P, seed) in SIZES.items():
        pts = ko.pooled(I, P, seed)
        c0 = pts[ko.fps32(pts, P)]
        out[name] = (pts, c0, ko.run(pts, c0), ko.lloyd64(pts, c0))
    return out


@pytest.mark.parametrize("name", list(SIZES))
def test_restatement_agrees_with_fp64_lloyd_and_kmeans2(runs, name):
    """same iteration count, same labels; centres differ by the fp32 rounding of a coordinate of a few hundred (half an ulp of
    256..512 is 1.5e-5) and what 24 iterations carry of it; scipy's kmeans2 from the same centres, run for as many iterations,
    gives the fp64 Lloyd's centres to fp64 rounding (no empty cluster on these inputs: kmeans2 would warn, and that is an error
    here)"""
    from scipy.cluster.vq import kmeans2
    pts, c0, r, o = runs[name]
    assert r["n_iter"] == o["n_iter"] and 2 < r["n_iter"] < 100
    assert r["n_empty"] == 0 and np.array_equal(r["labels"], o["labels"])
    err = np.abs(r["centres"] - o["centres"]).max()
    print(name, "iterations", r["n_iter"], "max centre difference", err, "inertia", r["inertia"], o["inertia"])
    assert err <= 4 * 2.0 ** -16
    assert abs(r["inertia"] - o["inertia"]) <= 1e-6 * o["inertia"]
    assert all(b <= a for a, b in zip(o["inertias"], o["inertias"][1:])) and o["inertia"] < o["inertias"][0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c2, l2 = kmeans2(pts.astype(np.float64), c0.astype(np.float64), iter=o["n_iter"], minit="matrix")
    np.testing.assert_allclose(c2, o["centres"], rtol=0, atol=1e-10)
    assert np.array_equal(l2, o["labels"])


def test_fixed_point_sums_do_not_depend_on_the_order_of_the_points(runs):
    pts, c0, _, _ = runs["12x37"]
    perm = np.random.default_rng(1).permutation(len(pts))
    a, b = ko.Restatement(pts, c0), ko.Restatement(pts[perm], c0)
    a.step()
    b.step()
    assert (a.s, a.si) == (b.s, b.si) and np.array_equal(a.labels[perm], b.labels)
    assert np.array_equal(a.c.view(np.uint32), b.c.view(np.uint32)) and np.array_equal(a.counts, b.counts)
    assert a.inertia == b.inertia and a.n_changed == b.n_changed == len(pts)
    # the scale leaves n of the largest values inside int64, and every fp32 coordinate of these clouds is represented exactly
    assert abs(int(a.fixed.max())) * len(pts) < 2 ** 63
    assert np.array_equal(np.ldexp(a.fixed.astype(np.float64), -a.s).astype(np.float32), pts)


def test_scales_and_rounding_rule():
    pts = np.array([[0.75, -300.5, 2.0], [1.0, 2.0, 3.0], [5.0, 6.0, 7.0]], np.float32)
    s, si = ko.scales(pts, pts[:1])
    assert (s, si) == (62 - 2 - 9, 62 - 2 - 22)        # 300.5 < 2^9, n = 3 -> L = 2
    assert ko.scales(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32)) == (62, 58)
    assert ko.scales(pts, np.array([[1024., 0., 0.]], np.float32))[0] == 62 - 2 - 11   # the centres count: 1024 = 0.5 * 2^11
    assert ko.to_fixed(np.array([0.5, 1.5, 2.5, -0.5], np.float32), 0).tolist() == [0, 2, 2, 0]   # round half to even
    assert ko.block_sum(np.arange(3000.)) == 3000 * 2999 / 2


def test_restatement_argument_checks_and_stopping_rule(runs):
    pts, c0, r, _ = runs["12x37"]
    for bad_p, bad_c in ((pts[:, :2], c0), (pts, c0[None]), (pts[:5], c0), (pts, np.zeros((0, 3), np.float32)),
                         (np.where(np.arange(len(pts))[:, None] == 3, np.nan, pts), c0)):
        with pytest.raises(ValueError):
            ko.Restatement(bad_p, bad_c)
    # tol = 0: the run ends on the iteration that changes no label, and only there
    z = ko.Restatement(pts, c0, tol=0.)
    changed = []
    while z.active:
        z.step()
        changed.append(z.n_changed)
    assert changed[-1] == 0 and all(c > 0 for c in changed[:-1]) and z.shift == 0. and z.n_iter == len(changed)
    # a frozen item no longer changes
    before = (z.c.copy(), z.labels.copy(), z.n_iter)
    z.step()
    assert np.array_equal(before[0], z.c) and np.array_equal(before[1], z.labels) and before[2] == z.n_iter
    # a huge tolerance stops after the first iteration; max_iter = 1 as well; max_iter = 0 only assigns
    assert ko.run(pts, c0, tol=1e9)["n_iter"] == 1 and ko.run(pts, c0, max_iter=1)["n_iter"] == 1
    zero = ko.run(pts, c0, max_iter=0)
    assert zero["n_iter"] == 0 and np.array_equal(zero["centres"], c0) and zero["inertia"] == r["inertias"][0]
    # sklearn's threshold: tol * mean of the per-axis variances
    assert abs(ko.threshold(pts, 1e-4) - 1e-4 * pts.astype(np.float64).var(0).mean()) <= 1e-12 * ko.threshold(pts, 1e-4)
    # an emptied cluster keeps its centre: two coincident centres, the higher index gets nothing
    c = c0.copy()
    c[5] = c[2]
    e = ko.Restatement(pts, c)
    e.step()
    assert e.counts[5] == 0 and e.n_empty == 1 and np.array_equal(e.c[5], c[5]) and e.counts[2] > 0


@pytest.mark.parametrize("name", list(SIZES))
def test_fp32_labels_need_no_excuse_on_the_test_inputs(runs, name):
    """the GPU test excuses a point whose two best fp64 squared distances differ by less than 1e-5 relative (about forty times
    the fp32 rounding of the direct form) and allows 0.1 % of them: here, at the centres that test uses (the farthest-point
    centres and the converged ones), how many there are and that fp32 labels equal fp64 labels everywhere else"""
    pts, c0, r, _ = runs[name]
    for what, c in (("initial", c0), ("converged", r["centres"])):
        lab, best, second = ko.assign64(pts, c)
        excused = (second - best) < 1e-5 * second
        lab32 = ko.sq_dist(pts, c, np.float32).argmin(1)
        print(name, what, "excused", int(excused.sum()), "of", len(pts), "smallest relative gap", ((second - best) / second).min())
        assert excused.mean() <= 1e-3 and np.array_equal(lab32[~excused], lab[~excused])


# ------------------------------------------------------------------ the real-reference fixture
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "correspondences_ref.npz"))


def test_reference_fixture_is_self_consistent(golden):
    from fissure_segmentation_amd.utils.general_utils import inverse_affine_transform
    inp = ko.correspondence_inputs()
    I, O, P = ko.CORR_INSTANCES, ko.CORR_OBJECTS, ko.CORR_POINTS
    assert int(golden["seed"]) == ko.CORR_SEED and os.path.getsize(os.path.join(GOLDEN_DIR, "correspondences_ref.npz")) < 100_000
    for tag in ("simple_undo", "simple_keep", "kmeans_undo"):
        assert golden[f"{tag}_pcs"].shape == (I, O * P, 3) and golden[f"{tag}_fixed"].shape == (O * P, 3)
        assert golden[f"{tag}_labels"].tolist() == [1] * P + [2] * P
        assert golden[f"{tag}_is_applied"].tolist() == [tag.endswith("keep")] * I
        for k in ("mean", "std", "hd", "cf"):
            assert golden[f"{tag}_{k}"].shape == (I, O) and np.isfinite(golden[f"{tag}_{k}"]).all()
    assert np.array_equal(golden["simple_undo_fixed"], inp["fixed_pcs"].reshape(-1, 3))
    assert not np.array_equal(golden["kmeans_undo_fixed"], golden["simple_undo_fixed"])
    # the evaluation always uses the cloud with the affine pre-registration undone
    for k in ("mean", "std", "hd", "cf"):
        assert np.array_equal(golden[f"simple_undo_{k}"], golden[f"simple_keep_{k}"])
    for i, t in enumerate(inp["transforms"]):
        back = inverse_affine_transform(golden["simple_keep_pcs"][i], t["scale"], t["rotation"], t["translation"])
        np.testing.assert_allclose(back, golden["simple_undo_pcs"][i], rtol=0, atol=1e-9)
    # the registration of the inputs succeeded: the corresponding points lie on the instances' meshes to a fraction of a millimetre
    assert golden["simple_undo_mean"].max() < 1. and golden["simple_undo_hd"].max() < 5.
    # parity of the kNN interpolation needs the same 5 neighbours in fp32 and fp64: the 5th and 6th distances are apart, and the
    # nearest distance is either exactly 0 (a k-means centre of a single point: the weight 1 / 1e-8 then owns the mean in any
    # precision) or far from the 1e-8 that is added to it
    for tag in ("simple_undo", "kmeans_undo"):
        q = golden[f"{tag}_fixed"].reshape(O, P, 3)
        for i in range(I):
            for o in range(O):
                d = np.sort(np.sqrt(((q[o][:, None] - inp["moved_pcs"][i, o][None]) ** 2).sum(-1)), 1)
                assert ((d[:, 5] - d[:, 4]) / d[:, 5]).min() > 5e-5 and ((d[:, 0] == 0) | (d[:, 0] > 1e-3)).all()


def test_batched_affine_undo_equals_the_single_one():
    from fissure_segmentation_amd.shape_model.generate_corresponding_points import inverse_affine_transform_batch
    from fissure_segmentation_amd.utils.general_utils import inverse_affine_transform
    inp = ko.correspondence_inputs()
    pcs = torch.from_numpy(inp["moved_pcs"][:, 0])
    tr = inp["transforms"]
    s = torch.tensor([t["scale"] for t in tr], dtype=torch.float64)
    R = torch.from_numpy(np.stack([t["rotation"] for t in tr]))
    tl = torch.from_numpy(np.stack([t["translation"] for t in tr]))
    got = inverse_affine_transform_batch(pcs, s, R, tl)
    for i in range(len(tr)):
        torch.testing.assert_close(got[i], inverse_affine_transform(pcs[i], s[i], R[i], tl[i]), rtol=0, atol=1e-11)
        assert torch.equal(got[i:i + 1], inverse_affine_transform_batch(pcs[i:i + 1], s[i:i + 1], R[i:i + 1], tl[i:i + 1]))


# ------------------------------------------------------------------ refusals before any launch
def test_python_refusals():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.shape_model import generate_corresponding_points as gcp
    pts, cen = torch.zeros(2, 10, 3), torch.zeros(2, 4, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.kmeans(pts, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.kmeans(pts, init=cen)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.kmeans_step(pts, cen)
    with pytest.raises(TypeError):
        F_hip.kmeans(pts.numpy(), 4)
    for bad in (dict(points=pts[..., :2]), dict(points=pts[None]), dict(points=pts.long()), dict(n_clusters=11), dict(n_clusters=0),
                dict(n_clusters=None), dict(n_clusters=4097, points=torch.zeros(1, 5000, 3)), dict(init="random"),
                dict(init=cen[:1]), dict(init=cen, n_clusters=5), dict(init=torch.zeros(2, 11, 3)), dict(max_iter=-1),
                dict(max_iter=2.5), dict(tol=-1.), dict(start=10)):
        with pytest.raises(ValueError):
            F_hip.kmeans(**{**dict(points=pts, n_clusters=4), **bad})
    for bad_p, bad_c in ((pts[0], cen), (pts, cen[:1]), (pts, torch.zeros(2, 11, 3)), (pts, cen[..., :2])):
        with pytest.raises(ValueError):
            F_hip.kmeans_step(bad_p, bad_c)
    assert gcp.CORRESPONDENCE_MODES == ["kmeans", "cluster", "simple"]
    a4, a3 = np.zeros((2, 1, 6, 3)), np.zeros((1, 6, 3))
    call = lambda **kw: gcp.data_set_correspondences(a3, [[None]] * 2, a4, [{}] * 2, a4, a4, None, None, **kw)   # noqa: E731
    with pytest.raises(NotImplementedError, match="OPTICS"):
        call()                                     # the reference's default mode is 'cluster'
    with pytest.raises(NotImplementedError, match="Parzen mode is unfinished"):
        call(mode="parzen")
    with pytest.raises(ValueError, match="No mode named nope."):
        call(mode="nope")
    with pytest.raises(NotImplementedError, match="tps.*out of scope"):
        call(mode="simple", interpolation_mode="tps")
    with pytest.raises(ValueError, match="interpolation_mode must be one of"):
        call(mode="simple", interpolation_mode="linear")
    with pytest.raises(RuntimeError, match="GPU only"):
        t3, t4 = torch.from_numpy(a3), torch.from_numpy(a4)
        gcp.data_set_correspondences(t3, [[None]] * 2, t4, [{}] * 2, t4, t4, None, None, mode="simple")


def test_host_side_checks_of_the_entry_points():
    from fissure_segmentation_amd import _lib
    q = _lib.lib.fsg_kmeans_workspace_bytes
    assert q(1, 100, 37) == 37 * 24 + 38 * 4 + 48 and q(3, 1 << 20, 1024) == 3 * (1024 * 28 + 48) and q(0, 5, 5) == 0
    assert q(2, 70, 4096) % 8 == 0 and q(2, 70, 37) % 8 == 0
    step = lambda *a: _lib.call("fsg_kmeans_step_f32", *a)   # noqa: E731
    for B, n, K in ((1, 0, 1), (1, 5, 0), (1, 5, 6), (1, 5000, 4097), (-1, 5, 2), (1, (1 << 24) + 1, 2)):
        with pytest.raises(RuntimeError, match="bad shape"):
            step(8, 8, 8, B, n, K, 8, 1 << 30, None, None, None, None)
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_kmeans_prepare_f32", 8, 8, B, n, K, 0., 8, 1 << 30, None)
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("fsg_kmeans_assign_f32", 8, 8, 8, B, n, K, 8, 1 << 30, None, None, None, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        step(None, 8, 8, 1, 5, 2, 8, 1 << 30, None, None, None, None)
    with pytest.raises(RuntimeError, match="workspace of 63 bytes"):
        step(8, 8, 8, 1, 5, 2, 8, 63, None, None, None, None)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        step(8, 8, 8, 1, 5, 2, 4, 1 << 30, None, None, None, None)
    with pytest.raises(RuntimeError, match="tol"):
        _lib.call("fsg_kmeans_prepare_f32", 8, 8, 1, 5, 2, -1., 8, 1 << 30, None)
    step(None, None, None, 0, 5, 2, None, 0, None, None, None, None)   # an empty batch is no error and launches nothing


def test_reference_import_name_resolves():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from shape_model.generate_corresponding_points import CORRESPONDENCE_MODES, data_set_correspondences  # noqa: F401
    finally:
        sys.modules.clear()
        sys.modules.update(saved)
