"""CPU tests of the DSEG-AE port: the oracles themselves (tests/dseg_ae_oracle.py), the real-reference fixture
tests/golden/dseg_ae_extend.npz against the fp64 oracle with the draws replayed from its seed, the model's constructor /
checkpoint contract and every refusal that happens before a launch."""
import os

import numpy as np
import pytest
import torch

import dseg_ae_oracle as do
from golden_util import GOLDEN_DIR


# ------------------------------------------------------------------ the oracles
def test_partition_oracle_is_a_stable_split():
    rng = np.random.default_rng(3)
    B, N, L = 3, 257, 4
    labels = rng.integers(-1, L + 3, (B, N))
    x = rng.standard_normal((B, 5, N)).astype(np.float32)
    counts, offset, xyz, src = do.partition(labels, x, L, first_label=1)
    assert counts.sum() == ((labels >= 1) & (labels <= L)).sum() == offset[-1] and np.all(np.diff(offset) >= 0)
    st = 0
    for g, en in enumerate(offset):
        b, l = divmod(g, L)
        rows = src[st:en]
        assert np.all(np.diff(rows) > 0) and np.all(labels[b, rows] == l + 1) and len(rows) == counts[b, l]
        assert np.array_equal(xyz[st:en], x[b, :3, :].T[rows])
        st = en
    assert not xyz[offset[-1]:].any() and not src[offset[-1]:].any()


def test_extend_oracle_statistics_and_rows():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(4)
    lens, targets = [1, 2, 65, 300], [4, 2, 70, 100]
    xyz = rng.random((sum(lens), 3)).astype(np.float32)
    ends = np.cumsum(lens)
    pads = [max(t - n, 0) for n, t in zip(lens, targets)]
    src = np.concatenate([rng.integers(0, n, p) for n, p in zip(lens, pads)])
    direction, z = rng.standard_normal((sum(pads), 3)), rng.standard_normal(sum(pads))
    out, new_ends, stats = do.extend(xyz, ends, targets, src, direction, z)
    assert new_ends.tolist() == np.cumsum([max(n, t) for n, t in zip(lens, targets)]).tolist()
    assert stats[0].tolist() == [0, 0] and np.isfinite(stats).all() and np.isfinite(out).all()
    p = 0
    for g, (n, pad) in enumerate(zip(lens, pads)):
        seg, o = xyz[ends[g] - n:ends[g]].astype(np.float64), out[new_ends[g] - n - pad:new_ends[g]]
        assert np.array_equal(o[:n], seg)
        if n >= 2:
            nn = cKDTree(seg).query(seg, k=2)[0][:, 1]
            np.testing.assert_allclose(stats[g], [nn.mean(), nn.std(ddof=1)], rtol=1e-12)
        # a padded row lies at distance |z std + mean| from its source, along the direction
        step = o[n:] - seg[src[p:p + pad]]
        np.testing.assert_allclose(np.linalg.norm(step, axis=1), np.abs(z[p:p + pad] * stats[g, 1] + stats[g, 0]), atol=1e-12)
        if n >= 2:
            unit = direction[p:p + pad] / np.linalg.norm(direction[p:p + pad], axis=1, keepdims=True)
            np.testing.assert_allclose(step, unit * (z[p:p + pad] * stats[g, 1] + stats[g, 0])[:, None], atol=1e-12)
        p += pad
    # the fp32 restatement stays within fp32 rounding of the oracle
    o32 = do.extend(xyz, ends, targets, src, direction.astype(np.float32), z.astype(np.float32), np.float32)[0]
    assert o32.dtype == np.float32 and np.abs(o32 - out).max() < 1e-5


def test_fps_oracle_rules():
    rng = np.random.default_rng(5)
    lens = [40, 0, 7]
    xyz = rng.integers(0, 4, (sum(lens), 3)).astype(np.float32)       # a tiny grid: duplicates and ties everywhere
    ends = np.cumsum(lens)
    got = do.fps(xyz, ends, [40, 3, 7], starts=[17, 0, 6])
    assert got[0][0] == 17 and got[2][0] == 40 + 6 and got[1].tolist() == [0, 0, 0]
    for g, (st, en) in enumerate(zip([0, 40, 40], ends)):
        if en == st:
            continue
        pts, idx = xyz[st:en].astype(np.float64), got[g] - st
        md = np.full(en - st, np.inf)
        for t in range(len(idx) - 1):
            md = np.minimum(md, ((pts - pts[idx[t]]) ** 2).sum(1))
            assert md[idx[t + 1]] == md.max() and idx[t + 1] == np.flatnonzero(md == md.max())[0]
    # a prefix of a longer run is the shorter run
    assert np.array_equal(do.fps(xyz, ends, [5, 0, 2], starts=[17, 0, 6])[0], got[0][:5])


# ------------------------------------------------------------------ the real-reference fixture
def test_golden_extension_against_the_fp64_oracle():
    path = os.path.join(GOLDEN_DIR, "dseg_ae_extend.npz")
    g = np.load(path)
    assert os.path.getsize(path) < 300_000 and sorted(g.files) == ["n", "oracle_out", "oracle_stats", "ref_error", "ref_out", "ref_stats",
                                                                    "seed", "target"]
    assert (int(g["seed"]), int(g["n"]), int(g["target"])) == (do.GOLDEN_SEED, do.GOLDEN_N, do.GOLDEN_TARGET)
    points, src, direction, z = do.golden_draws()
    pts = points[0].numpy()
    assert len(np.unique(pts, axis=0)) == do.GOLDEN_N and np.array_equal(g["ref_out"][:do.GOLDEN_N], pts)
    out, new_ends, stats = do.extend(pts, [do.GOLDEN_N], do.GOLDEN_TARGET, src.numpy(), direction.numpy(), z.numpy())
    assert new_ends.tolist() == [do.GOLDEN_TARGET] and not np.isnan(g["ref_out"]).any()
    np.testing.assert_allclose(out, g["oracle_out"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(stats[0], g["oracle_stats"], rtol=1e-13)
    err = np.abs(g["ref_out"].astype(np.float64) - out).max()
    print("reference's fp32 error", err, "recorded", float(g["ref_error"]), "stats", stats[0], g["ref_stats"])
    assert abs(err - float(g["ref_error"])) <= 1e-12 and 0 < err < 4 * do.FLOOR       # coordinates in [0, 1): a few fp32 ulps
    np.testing.assert_allclose(g["ref_stats"], stats[0], rtol=1e-5)      # the reference's fp32 mean and deviation


# ------------------------------------------------------------------ the model: constructor, checkpoints, alias
def _checkpoints(tmp_path, decode_mesh=True):
    from golden_util import fill_state_dict
    from fissure_segmentation_amd.models.dgcnn import DGCNNSeg
    from fissure_segmentation_amd.models.folding_net import DGCNNFoldingNet
    seg = fill_state_dict(DGCNNSeg(k=8, in_features=3, num_classes=4), 11)
    ae = fill_state_dict(DGCNNFoldingNet(k=8, n_embedding=32, shape_type='plane', n_input_points=64, decode_mesh=decode_mesh), 12)
    seg_path, ae_path = str(tmp_path / "seg.pth"), str(tmp_path / "ae.pth")
    seg.save(seg_path)
    ae.save(ae_path)
    return seg, ae, seg_path, ae_path


def test_constructor_config_and_checkpoint_round_trip(tmp_path):
    from fissure_segmentation_amd.dseg_ae_regularization import RegularizedSegDGCNN
    seg, ae, seg_path, ae_path = _checkpoints(tmp_path)
    model = RegularizedSegDGCNN(seg_path, ae_path, n_points_seg=256, n_points_ae=64, random_extend=True)
    assert model.config == dict(seg_model=seg_path, ae=ae_path, n_points_seg=256, n_points_ae=64, sample_mode='farthest',
                                random_extend=True)
    keys = list(model.state_dict())
    assert keys and all(k.startswith(("seg_model.", "ae.")) for k in keys)
    assert {k[len("seg_model."):] for k in keys if k.startswith("seg_model.")} == set(seg.state_dict())
    assert {k[len("ae."):] for k in keys if k.startswith("ae.")} == set(ae.state_dict())
    for k, v in seg.state_dict().items():
        assert torch.equal(model.state_dict()["seg_model." + k], v)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    path = str(tmp_path / "model.pth")
    model.save(path)
    ckpt = torch.load(path)
    assert ckpt["config"] == model.config and not any(k.endswith(".grid") for k in ckpt["model_state"])
    again = RegularizedSegDGCNN.load(path, 'cpu')
    assert again.config == model.config and (again.n_points_seg, again.n_points_ae, again.sample_mode, again.random_extend) == \
        (256, 64, 'farthest', True)
    for k, v in model.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k
    assert again.seg_model.num_classes == 4 and again.ae.encoder.k == 8 and again.ae.decoder.m == 64


def test_mode_errors_come_before_any_launch(tmp_path):
    from fissure_segmentation_amd.dseg_ae_regularization import RegularizedSegDGCNN
    _, _, seg_path, ae_path = _checkpoints(tmp_path)
    x, seg = torch.zeros(1, 3, 50), torch.zeros(1, 50, dtype=torch.int64)
    nope = RegularizedSegDGCNN(seg_path, ae_path, 256, 64, sample_mode='nope')
    acc = RegularizedSegDGCNN(seg_path, ae_path, 256, 64, sample_mode='accumulate')
    for call in (nope.reconstruct, nope.reconstruct_packed):
        with pytest.raises(NotImplementedError, match="Sampling mode nope not implemented."):
            call(x, seg)
    for call in (acc.reconstruct, acc.reconstruct_packed):
        with pytest.raises(NotImplementedError, match="Hidden output not implemented for accumulate sampling."):
            call(x, seg, return_hidden=True)
    with pytest.raises(ValueError, match="one cloud at a time"):
        acc.reconstruct(torch.zeros(2, 3, 50), torch.zeros(2, 50, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):
        acc.reconstruct(x, seg)


def test_reference_import_name_resolves():
    import sys
    import fissure_segmentation_amd as fsg
    saved = dict(sys.modules)
    try:
        fsg.install_reference_aliases()
        from dseg_ae_regularization import (RegularizedSegDGCNN, farthest_point_sampling, random_extend_points,  # noqa: F401
                                            reconstruction_metrics)
        from fissure_segmentation_amd.utils import general_utils
        assert farthest_point_sampling is general_utils.farthest_point_sampling
    finally:
        sys.modules.clear()
        sys.modules.update(saved)


# ------------------------------------------------------------------ refusals before any launch
def test_python_refusals():
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.dseg_ae_regularization import random_extend_points
    lab, x = torch.zeros(2, 10, dtype=torch.int64), torch.zeros(2, 3, 10)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.label_partition(lab, x, 3)
    for bad in (dict(labels=lab[0]), dict(x=x[:, :2]), dict(x=x[:1]), dict(x=x[..., :9]), dict(num_labels=0), dict(num_labels=17)):
        with pytest.raises(ValueError):
            F_hip.label_partition(**{**dict(labels=lab, x=x, num_labels=3), **bad})
    with pytest.raises(TypeError):
        F_hip.label_partition(lab.to(torch.int16), x, 3)
    xyz = torch.zeros(10, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.segment_jitter_extend(xyz, [4, 10], 8, torch.zeros(6, dtype=torch.int32), torch.zeros(6, 3), torch.zeros(6))
    with pytest.raises(RuntimeError, match="GPU only"):
        F_hip.fps_start(xyz, torch.tensor([10]), torch.tensor([4]), 4)
    assert random_extend_points(torch.zeros(1, 10, 3), 10).shape == (1, 10, 3)      # nothing to pad: the input, on any device
    with pytest.raises(RuntimeError, match="GPU only"):
        random_extend_points(torch.rand(1, 10, 3), 12)


def test_host_side_checks_of_the_entry_points():
    from fissure_segmentation_amd import _lib
    q = _lib.lib.fsg_label_partition_workspace_bytes
    assert q(1, 1, 1) == 4 and q(3, 1025, 16) == 3 * 2 * 16 * 4 and q(0, 5, 5) == 0 and q(2, 1024, 3) == 2 * 3 * 4
    part = lambda *a: _lib.call("fsg_label_partition", *a)   # noqa: E731
    for B, C, N, L in ((0, 3, 5, 1), (1, 2, 5, 1), (1, 3, 0, 1), (1, 3, 5, 0), (1, 3, 5, 17), (1 << 16, 3, 1 << 15, 1)):
        with pytest.raises(RuntimeError, match="bad shape"):
            part(8, 0, 8, B, C, N, 1, L, 8, 8, 8, 8, 8, 1 << 40, None)
    with pytest.raises(RuntimeError, match="label_kind 3"):
        part(8, 3, 8, 1, 3, 5, 1, 1, 8, 8, 8, 8, 8, 1 << 40, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        part(None, 0, 8, 1, 3, 5, 1, 1, 8, 8, 8, 8, 8, 1 << 40, None)
    with pytest.raises(RuntimeError, match="workspace of 3 bytes"):
        part(8, 0, 8, 1, 3, 5, 1, 1, 8, 8, 8, 8, 8, 3, None)
    ext = lambda *a: _lib.call("fsg_segment_jitter_extend_f32", *a)   # noqa: E731
    for G, n, n_new in ((0, 5, 5), (1, 0, 0), (1, 5, 4)):
        with pytest.raises(RuntimeError, match="bad shape"):
            ext(8, 8, 8, 8, 8, 8, 8, G, n, n_new, 8, 8, None)
    with pytest.raises(RuntimeError, match="3 padded rows without draws"):
        ext(8, 8, 8, 8, None, 8, 8, 1, 5, 8, 8, 8, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        ext(8, 8, None, 8, 8, 8, 8, 1, 5, 8, 8, 8, None)
    fps = lambda *a: _lib.call("fsg_fps_start_f32", *a)   # noqa: E731
    for b, n in ((0, 5), (1, 0)):
        with pytest.raises(RuntimeError, match="bad shape"):
            fps(8, 8, 8, None, b, n, 8, 8, None)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        fps(8, 8, 8, None, 1, 5, None, 8, None)
