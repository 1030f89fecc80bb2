"""GPU tests of the DSEG-AE port (csrc/dseg_ae.hip, fissure_segmentation_amd/dseg_ae_regularization.py).

Partition and farthest point sampling are integer-exact or order-exact: bitwise against the oracles of tests/dseg_ae_oracle.py.
The extension is held to the house bar against the fp64 oracle: 4 x the error of the oracle's own fp32 restatement on the same
input, floor 4.8e-7 of the coordinate magnitude; the real-reference case to 4 x the reference's recorded error.  The pipeline is
compared with the per-object loop of the reference written over this package's public pieces, with the same draws."""
import numpy as np
import pytest
import torch

import dseg_ae_oracle as do
from golden_util import fill_state_dict, load

pytestmark = pytest.mark.gpu

FLOOR = do.FLOOR


def G(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------ partition: bitwise
PART_N = [1, 63, 64, 65, 1024, 1025, 20 * 1024 + 7]     # the last: 3 x 21 (item, tile) rows of counts, 16 are walked at a time
PART_DTYPES = {"u8": (torch.uint8, np.uint8), "i32": (torch.int32, np.int32), "i64": (torch.int64, np.int64)}


def _labels(rng, B, N, L, first, np_dtype, mode):
    if mode == "background":
        lab = np.full((B, N), first - 1 if first > 0 else first + L, np.int64)
    elif mode == "single":
        lab = np.full((B, N), first + L - 1, np.int64)
    else:   # every object, and labels on both sides of the range
        lab = rng.integers(first - 2, first + L + 2, (B, N))
        if np_dtype is np.int64:
            lab[rng.random((B, N)) < 0.05] = (1 << 40) + first      # equal to an object's label in the low 32 bits only
    if np_dtype is np.uint8:
        lab = np.where(lab < 0, 255, lab)
    return lab.astype(np_dtype)


@pytest.mark.parametrize("kind", list(PART_DTYPES))
@pytest.mark.parametrize("N", PART_N)
def test_label_partition_is_the_stable_split(device, N, kind):
    from fissure_segmentation_amd import functional as F_hip
    t_dtype, np_dtype = PART_DTYPES[kind]
    rng = np.random.default_rng(N)
    for B in (1, 3):
        for L, first in ((1, 1), (3, 1), (16, 2), (3, 0)):
            for mode in ("mixed", "background", "single"):
                lab = _labels(rng, B, N, L, first, np_dtype, mode)
                x = rng.standard_normal((B, 4, N)).astype(np.float32)
                want = do.partition(lab, x, L, first)
                got = [t.cpu().numpy() for t in F_hip.label_partition(G(lab, device), G(x, device), L, first_label=first)]
                for name, w, g in zip(("counts", "offset", "xyz", "src"), want, got):
                    assert w.dtype == g.dtype and w.shape == g.shape, (name, B, L, mode)
                    assert np.array_equal(w.view(np.uint32) if w.dtype == np.float32 else w,
                                          g.view(np.uint32) if g.dtype == np.float32 else g), (name, B, L, first, mode)
                if mode == "background":
                    assert want[1][-1] == 0
                if mode == "single":
                    assert want[0][:, -1].tolist() == [N] * B
                if B == 3 and mode == "mixed":      # an item alone gives the segments it gives in the batch
                    for b in range(B):
                        alone = [t.cpu().numpy() for t in F_hip.label_partition(G(lab[b:b + 1], device), G(x[b:b + 1], device), L,
                                                                                first_label=first)]
                        st, en = (got[1][b * L - 1] if b else 0), got[1][(b + 1) * L - 1]
                        assert np.array_equal(alone[0][0], got[0][b]) and alone[1][-1] == en - st
                        assert np.array_equal(alone[2][:en - st].view(np.uint32), got[2][st:en].view(np.uint32))
                        assert np.array_equal(alone[3][:en - st], got[3][st:en])


# ------------------------------------------------------------------ extension: the house bar against the fp64 oracle
EXT_LENS = [2, 3, 64, 65, 700]
EXT_TARGETS = [1, 3, 100, 65, 1024]       # below, equal, above, equal, above


@pytest.fixture(scope="module")
def ext_case():
    rng = np.random.default_rng(77)
    xyz = rng.uniform(-1, 1, (sum(EXT_LENS), 3)).astype(np.float32)
    pads = [max(t - n, 0) for n, t in zip(EXT_LENS, EXT_TARGETS)]
    src = np.concatenate([rng.integers(0, n, p) for n, p in zip(EXT_LENS, pads)]).astype(np.int32)
    direction = rng.standard_normal((sum(pads), 3)).astype(np.float32)
    z = rng.standard_normal(sum(pads)).astype(np.float32)
    ends = np.cumsum(EXT_LENS)
    o64 = do.extend(xyz, ends, EXT_TARGETS, src, direction, z)
    o32 = do.extend(xyz, ends, EXT_TARGETS, src, direction, z, np.float32)
    return dict(xyz=xyz, ends=ends, pads=pads, src=src, direction=direction, z=z, o64=o64, o32=o32)


def test_segment_jitter_extend_against_the_oracle(device, ext_case):
    from fissure_segmentation_amd import functional as F_hip
    c = ext_case
    out, new_off, stats = F_hip.segment_jitter_extend(G(c["xyz"], device), c["ends"].tolist(), EXT_TARGETS, G(c["src"], device),
                                                      G(c["direction"], device), G(c["z"], device))
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    o64, e64, s64 = c["o64"]
    o32, _, s32 = c["o32"]
    assert new_off.cpu().numpy().tolist() == e64.tolist() and out.shape == o64.shape and not np.isnan(out).any()
    bar = max(4 * np.abs(o32.astype(np.float64) - o64).max(), FLOOR * np.abs(c["xyz"]).max())
    err = np.abs(out.astype(np.float64) - o64).max()
    bar_s = max(4 * np.abs(s32.astype(np.float64) - s64).max(), FLOOR * np.abs(s64).max())
    err_s = np.abs(stats.astype(np.float64) - s64).max()
    print("extension: error", err, "bar", bar, "statistics: error", err_s, "bar", bar_s)
    assert err <= bar and err_s <= bar_s
    # the segment itself is copied
    p = 0
    for g, n in enumerate(EXT_LENS):
        st = e64[g] - max(n, EXT_TARGETS[g])
        assert np.array_equal(out[st:st + n].view(np.uint32), c["xyz"][c["ends"][g] - n:c["ends"][g]].view(np.uint32))
        # several segments in one launch equal each alone, bit for bit
        pad = c["pads"][g]
        a_out, _, a_stats = F_hip.segment_jitter_extend(G(c["xyz"][c["ends"][g] - n:c["ends"][g]], device), [n], EXT_TARGETS[g],
                                                        G(c["src"][p:p + pad], device), G(c["direction"][p:p + pad], device),
                                                        G(c["z"][p:p + pad], device))
        assert np.array_equal(a_out.cpu().numpy().view(np.uint32), out[st:e64[g]].view(np.uint32)), g
        assert np.array_equal(a_stats.cpu().numpy().view(np.uint32), stats[g:g + 1].view(np.uint32)), g
        p += pad


def test_short_segments_give_zero_statistics_not_nan(device):
    from fissure_segmentation_amd import functional as F_hip
    xyz = G(np.array([[1, 2, 3], [4, 5, 6], [4, 5, 7]], np.float32), device)
    src = torch.zeros(5, dtype=torch.int32, device=device)
    direction = torch.tensor([[0., 3., 4.]] * 5, device=device)
    # one point, no point, two points at distance 1; grown to 3, 2 and 3 rows
    out, new_off, stats = F_hip.segment_jitter_extend(xyz, [1, 1, 3], [3, 2, 3], src, direction, torch.ones(5, device=device))
    assert stats.cpu().tolist() == [[0, 0], [0, 0], [1, 0]] and new_off.cpu().tolist() == [3, 5, 8]
    o = out.cpu().numpy()
    assert np.array_equal(o[:3], np.array([[1, 2, 3]] * 3, np.float32))          # mean = std = 0: copies of the source
    assert not o[3:5].any()                                                       # nothing to copy from: zeros
    assert np.array_equal(o[5:7], np.array([[4, 5, 6], [4, 5, 7]], np.float32))
    np.testing.assert_allclose(o[7], [4, 5.6, 6.8], rtol=0, atol=FLOOR * 7)        # one step of length 1 along (0, 3, 4) / 5


def test_random_extend_points_golden_case(device):
    """the real reference's output (tests/golden/dseg_ae_extend.npz) with its draws replayed from the seed: ours against the
    fp64 oracle within 4 x the reference's own recorded fp32 error"""
    from fissure_segmentation_amd.dseg_ae_regularization import random_extend_points
    g = load("dseg_ae_extend")
    points, src, direction, z = do.golden_draws()
    out = random_extend_points(points.to(device), do.GOLDEN_TARGET, draws=(src, direction.to(device), z.to(device)))
    assert out.shape == (1, do.GOLDEN_TARGET, 3) and out.dtype == torch.float32
    out = out[0].cpu().numpy().astype(np.float64)
    err, bar = np.abs(out - g["oracle_out"]).max(), 4 * float(g["ref_error"])
    print("golden extension: error", err, "bar", bar, "distance to the reference's output", np.abs(out - g["ref_out"]).max())
    assert err <= bar
    # per item statistics: a batch of two clouds gives each what it gives alone
    two = torch.cat([points, points.flip(1) * 0.5]).to(device)
    d2, z2 = torch.cat([direction, direction]).to(device), torch.cat([z, -z]).to(device)
    both = random_extend_points(two, do.GOLDEN_TARGET, draws=(src, d2, z2))
    for b in range(2):
        alone = random_extend_points(two[b:b + 1], do.GOLDEN_TARGET, draws=(src, d2[b:b + 1], z2[b:b + 1]))
        assert torch.equal(alone[0], both[b])


# ------------------------------------------------------------------ farthest point sampling with a start
FPS_LENS = [2049, 0, 100, 4096, 4097, 8193, 16384, 16385]       # an empty and a short segment among them; the last: the fallback
FPS_STARTS = {"first": lambda n: 0, "middle": lambda n: n // 2, "last": lambda n: max(n - 1, 0)}


@pytest.fixture(scope="module")
def fps_grid():
    """integer coordinates in [0, 1024): every squared distance is exact in fp32, ties are plentiful; the fp64 oracle run to
    m = len once per start (a shorter run is its prefix)"""
    rng = np.random.default_rng(9)
    xyz = rng.integers(0, 1024, (sum(FPS_LENS), 3)).astype(np.float32)
    xyz[-16385:-16385 + 64] = xyz[-1]       # a run of duplicates in the longest segment
    ends = np.cumsum(FPS_LENS)
    want = {name: do.fps(xyz, ends, FPS_LENS, [f(n) for n in FPS_LENS]) for name, f in FPS_STARTS.items()}
    return xyz, ends, want


@pytest.mark.parametrize("start", list(FPS_STARTS))
def test_fps_start_on_integer_grid_equals_the_oracle(device, fps_grid, start):
    from fissure_segmentation_amd import functional as F_hip
    xyz, ends, want = fps_grid
    x, off = G(xyz, device), G(ends.astype(np.int32), device)
    st = G(np.array([FPS_STARTS[start](n) for n in FPS_LENS], np.int32), device)
    for what, ms in (("1", [1] * len(FPS_LENS)), ("64", [64] * len(FPS_LENS)), ("len", FPS_LENS)):
        new_off = np.cumsum(ms).astype(np.int32)
        idx = F_hip.fps_start(x, off, G(new_off, device), int(new_off[-1]), st).cpu().numpy()
        q = 0
        for g, (n, m) in enumerate(zip(FPS_LENS, ms)):
            w = want[start][g][:m] if n else np.zeros(m, np.int64)      # samples asked of the empty segment: index 0
            assert len(w) == m
            assert np.array_equal(idx[q:q + m], w), (what, n, start, np.flatnonzero(idx[q:q + m] != w)[:4])
            q += m


def test_fps_start_null_start_equals_fps_bit_for_bit(device):
    """float inputs: with start = None (and with explicit zeros) the output equals `functional.fps`'s, whichever of its two
    kernels serves a segment"""
    from fissure_segmentation_amd import functional as F_hip
    rng = np.random.default_rng(10)
    xyz = rng.uniform(-1, 1, (sum(FPS_LENS), 3)).astype(np.float32)
    x, off = G(xyz, device), G(np.cumsum(FPS_LENS).astype(np.int32), device)
    for ms in ([64] * len(FPS_LENS), [min(n, 300) for n in FPS_LENS]):
        new_off = G(np.cumsum(ms).astype(np.int32), device)
        m = int(sum(ms))
        base = F_hip.fps(x, off, new_off, m)
        assert torch.equal(F_hip.fps_start(x, off, new_off, m), base)
        assert torch.equal(F_hip.fps_start(x, off, new_off, m, torch.zeros(len(FPS_LENS), dtype=torch.int32, device=device)), base)
    # a segment alone gives what it gives in the batch
    n0 = sum(FPS_LENS[:5])
    seg = G(xyz[n0:n0 + 8193], device)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=device)   # noqa: E731
    alone = F_hip.fps_start(seg, one(8193), one(64), 64, one(77))
    st = torch.zeros(len(FPS_LENS), dtype=torch.int32, device=device)
    st[5] = 77
    new_off = G(np.cumsum([64] * len(FPS_LENS)).astype(np.int32), device)
    batch = F_hip.fps_start(x, off, new_off, 64 * len(FPS_LENS), st)
    assert torch.equal(alone + n0, batch[5 * 64:6 * 64]) and int(alone[0]) == 77


def test_out_of_range_start_and_source_rows_are_clamped(device):
    """include/fsg_hip.h: `start` and `src_idx` are clamped to their segment -- a negative value means the first row, one at
    or beyond the length the last; nothing outside the segment is read"""
    from fissure_segmentation_amd import functional as F_hip
    rng = np.random.default_rng(21)
    lens = [300, 5000]
    xyz = rng.integers(0, 1024, (sum(lens), 3)).astype(np.float32)
    ends = np.cumsum(lens)
    x, off = G(xyz, device), G(ends.astype(np.int32), device)
    new_off = G(np.array([32, 64], np.int32), device)
    st = lambda a, b: torch.tensor([a, b], dtype=torch.int32, device=device)   # noqa: E731
    for bad, good in (((-5, 5000), (0, 4999)), ((300, -1), (299, 0)), ((1 << 30, -(1 << 30)), (299, 0))):
        got = F_hip.fps_start(x, off, new_off, 64, st(*bad)).cpu().numpy()
        want = do.fps(xyz, ends, [32, 32], list(good))
        assert np.array_equal(got[:32], want[0]) and np.array_equal(got[32:], want[1]), bad
        assert got[0] == good[0] and got[32] == 300 + good[1]
    seg = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    direction, z = rng.standard_normal((6, 3)).astype(np.float32), rng.standard_normal(6).astype(np.float32)
    bad, good = np.array([-1, 40, 41, -(1 << 30), 1 << 30, 7], np.int32), np.array([0, 39, 39, 0, 39, 7], np.int32)
    a = F_hip.segment_jitter_extend(G(seg, device), [40], 46, G(bad, device), G(direction, device), G(z, device))[0]
    b = F_hip.segment_jitter_extend(G(seg, device), [40], 46, G(good, device), G(direction, device), G(z, device))[0]
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    o64 = do.extend(seg, [40], 46, good, direction, z)[0]
    o32 = do.extend(seg, [40], 46, good, direction, z, np.float32)[0]
    assert np.abs(a.cpu().numpy() - o64).max() <= max(4 * np.abs(o32 - o64).max(), FLOOR * np.abs(seg).max())


# ------------------------------------------------------------------ the pipeline
N_AE, K_AE, N_CLOUD = 64, 8, 600


def _models(tmp_path, decode_mesh, **kw):
    from fissure_segmentation_amd.dseg_ae_regularization import RegularizedSegDGCNN
    from fissure_segmentation_amd.models.dgcnn import DGCNNSeg
    from fissure_segmentation_amd.models.folding_net import DGCNNFoldingNet
    n_in = N_AE if decode_mesh else 2025        # the point decoder folds the fixed 45 x 45 plane
    seg = fill_state_dict(DGCNNSeg(k=K_AE, in_features=3, num_classes=4), 11)
    ae = fill_state_dict(DGCNNFoldingNet(k=K_AE, n_embedding=32, shape_type='plane', n_input_points=n_in, decode_mesh=decode_mesh), 12)
    seg.save(str(tmp_path / "seg.pth"))
    ae.save(str(tmp_path / "ae.pth"))
    return RegularizedSegDGCNN(str(tmp_path / "seg.pth"), str(tmp_path / "ae.pth"), n_points_seg=256, n_points_ae=N_AE, **kw), n_in


def _cloud(seed, B, device):
    """clouds of 600 points and a hand-made segmentation: object 1 has 200 points (sampled), object 2 has 30 (extended, or a
    short auto-encoder input), object 3 has 5 (fewer than k: None)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, 3, N_CLOUD)).astype(np.float32)
    seg = np.zeros((B, N_CLOUD), np.int64)
    for b in range(B):
        perm = rng.permutation(N_CLOUD)
        seg[b, perm[:200]], seg[b, perm[200:230]], seg[b, perm[230:235]] = 1, 2, 3
    return G(x, device), G(seg, device)


def _ae_bar(model, n_in, decode_mesh, sampled, fix_graph=False):
    """the house bar for the auto-encoder's output on these inputs: 4 x the error of the CPU oracle's fp32 run against its fp64
    run, floor 4.8e-7 of the largest magnitude -- for the vertices and for the hidden code.  fix_graph: the fp64 run reuses the
    neighbour graphs of the fp32 run, so that the bar is rounding alone and not a neighbour that the two precisions rank
    differently"""
    from oracle import ref_cpu
    ref = ref_cpu.DGCNNFoldingNet(k=K_AE, n_embedding=32, n_input_points=n_in, decode_mesh=decode_mesh).eval()
    ref.load_state_dict({k: v.cpu() for k, v in model.ae.state_dict().items()})
    bar_v = bar_h = 0.
    real_knn = ref_cpu.knn_opensrc

    def encode_both(x32):
        graphs = []
        if not fix_graph:
            return ref.encoder(x32), ref.double().encoder(x32.double())
        try:
            ref_cpu.knn_opensrc = lambda x, k: graphs.append(real_knn(x, k)) or graphs[-1]
            h32 = ref.encoder(x32)
            replay = iter(graphs)
            ref_cpu.knn_opensrc = lambda x, k: next(replay)
            return h32, ref.double().encoder(x32.double())
        finally:
            ref_cpu.knn_opensrc = real_knn

    with torch.no_grad():
        for pts in sampled:
            x32 = pts.detach().cpu().float().transpose(1, 2).contiguous()
            h32, h64 = encode_both(x32)
            v64 = ref.decoder(h64)
            v32 = ref.float().decoder(h32)
            bar_v = max(bar_v, 4 * float((v32.double() - v64).abs().max()), FLOOR * float(v64.abs().max()))
            bar_h = max(bar_h, 4 * float((h32.double() - h64).abs().max()), FLOOR * float(h64.abs().max()))
    return bar_v, bar_h


@torch.no_grad()
def _loop(model, x, seg):
    """the reference's per-object loop (:62-106) over this package's public pieces"""
    from fissure_segmentation_amd.dseg_ae_regularization import farthest_point_sampling, random_extend_points
    meshes, points, hidden, index = [], [], [], []
    for obj in range(1, model.seg_model.num_classes):
        pts = x[:, :3].transpose(1, 2)[seg == obj].view(x.shape[0], -1, 3)
        if pts.shape[1] < model.ae.encoder.k:
            meshes.append(None), points.append(pts), hidden.append(None), index.append(None)
            continue
        if model.random_extend:
            pts = random_extend_points(pts, model.n_points_ae)
        if model.sample_mode == 'farthest':
            sampled, ind = farthest_point_sampling(pts, model.n_points_ae)
            mesh, h = model.ae(sampled.transpose(1, 2).contiguous(), return_hidden=True)
            points.append(sampled), hidden.append(h), index.append(ind)
        else:
            mesh = model.ae.predict_full_pointcloud(pts, model.n_points_ae, n_runs=10)
            points.append(pts), hidden.append(None), index.append(None)
        meshes.append(mesh)
    return meshes, points, hidden, index


@pytest.mark.parametrize("random_extend", [False, True], ids=["plain", "extend"])
@pytest.mark.parametrize("decode_mesh", [True, False], ids=["mesh", "points"])
def test_reconstruct_matches_the_per_object_loop(device, tmp_path, decode_mesh, random_extend):
    model, n_in = _models(tmp_path, decode_mesh, random_extend=random_extend)
    model = model.to(device).eval()
    x, seg = _cloud(5, 1, device)
    torch.manual_seed(123)
    meshes, points, hidden = model.reconstruct(x, seg, return_hidden=True)
    torch.manual_seed(123)
    packed = model.reconstruct_packed(x, seg, return_hidden=True)
    torch.manual_seed(123)
    l_meshes, l_points, l_hidden, l_index = _loop(model, x, seg)
    assert len(meshes) == len(points) == len(hidden) == 3 and meshes[2] is None and hidden[2] is None
    assert [p.shape for p in points] == [(1, N_AE, 3), (1, N_AE if random_extend else 30, 3), (1, 5, 3)]
    assert packed["valid"].tolist() == [True, True, False] and packed["group"].tolist() == [[0, 1], [0, 2], [0, 3]]
    ends = packed["points_offset"].tolist()
    bar_v, bar_h = _ae_bar(model, n_in, decode_mesh, [p for p in l_points[:2]])
    for o in range(3):
        assert torch.equal(points[o], l_points[o]), o                       # bit for bit
        if l_index[o] is not None:
            assert torch.equal(packed["index"][(ends[o - 1] if o else 0):ends[o]].cpu(), l_index[o].cpu().long()), o
        if o < 2:
            assert meshes[o].shape == l_meshes[o].shape == (1, 3, model.ae.decoder.m) and hidden[o].shape == l_hidden[o].shape == (1, 1, 32)
            ev, eh = float((meshes[o] - l_meshes[o]).abs().max()), float((hidden[o] - l_hidden[o]).abs().max())
            print("object", o + 1, "vertices: difference", ev, "bar", bar_v, "hidden: difference", eh, "bar", bar_h)
            assert ev <= bar_v and eh <= bar_h
            assert torch.equal(packed["vertices"][o], meshes[o][0].transpose(0, 1))
    # the sources of object 1's samples are the points that carry its label
    src = packed["source"][:200].long()
    assert bool((seg[0, src] == 1).all()) and bool((src[1:] > src[:-1]).all())


def test_reconstruct_packed_batch_equals_single_calls(device, tmp_path):
    model, n_in = _models(tmp_path, True, random_extend=True)
    model = model.to(device).eval()
    x, seg = _cloud(6, 2, device)
    torch.manual_seed(7)
    both = model.reconstruct_packed(x, seg, return_hidden=True)
    torch.manual_seed(7)
    singles = [model.reconstruct_packed(x[b:b + 1], seg[b:b + 1], return_hidden=True) for b in range(2)]
    assert both["group"].tolist() == [[b, o] for b in range(2) for o in (1, 2, 3)] and both["valid"].tolist() == [True, True, False] * 2
    assert torch.equal(both["points"], torch.cat([s["points"] for s in singles]))
    assert torch.equal(both["index"], torch.cat([s["index"] for s in singles]))
    assert torch.equal(both["source"], torch.cat([s["source"] for s in singles]))
    assert both["points_offset"].tolist() == singles[0]["points_offset"].tolist() + \
        (singles[1]["points_offset"] + singles[0]["points_offset"][-1]).tolist()
    ends = both["points_offset"].tolist()
    bar_v, bar_h = _ae_bar(model, n_in, True, [both["points"][(ends[g - 1] if g else 0):ends[g]][None] for g in (0, 1, 3, 4)])
    ev = float((both["vertices"] - torch.cat([s["vertices"] for s in singles])).abs().max())
    eh = float((both["hidden"] - torch.cat([s["hidden"] for s in singles])).abs().max())
    print("batch of two against two single calls: vertices", ev, "bar", bar_v, "hidden", eh, "bar", bar_h)
    assert ev <= bar_v and eh <= bar_h and not both["vertices"][[2, 5]].any()


def test_accumulate_mode_matches_its_loop(device, tmp_path):
    model, n_in = _models(tmp_path, True, sample_mode='accumulate')
    model = model.to(device).eval()
    x, seg = _cloud(8, 1, device)
    torch.manual_seed(31)
    meshes, points = model.reconstruct(x, seg)
    torch.manual_seed(31)
    l_meshes, l_points, _, _ = _loop(model, x, seg)
    assert meshes[2] is None and [p.shape[1] for p in points] == [200, 30, 5]
    # the bar of one run: the average of ten runs of it is no further off
    torch.manual_seed(31)
    runs = [l_points[0][:, torch.randperm(200, device=device)[:N_AE]] for _ in range(10)]
    bar_v, _ = _ae_bar(model, n_in, True, runs + [l_points[1]], fix_graph=True)
    for o in range(3):
        assert torch.equal(points[o], l_points[o])
        if o < 2:
            ev = float((meshes[o] - l_meshes[o]).abs().max())
            print("accumulate, object", o + 1, "difference", ev, "bar", bar_v)
            assert meshes[o].shape == l_meshes[o].shape == (1, N_AE, 3) and ev <= bar_v      # predict_full_pointcloud's layout


def test_return_meshes_wraps_the_same_vertices(device, tmp_path):
    """`DGCNNFoldingNet.return_meshes`: the auto-encoder hands out `mesh.Meshes`, and so do `reconstruct`'s lists, in both
    sampling modes, around the vertices of the plain run"""
    from fissure_segmentation_amd.mesh import Meshes
    x, seg = _cloud(12, 1, device)
    for mode in ('farthest', 'accumulate'):
        model, _ = _models(tmp_path, True, sample_mode=mode, random_extend=True)
        model = model.to(device).eval()
        torch.manual_seed(4)
        plain = model.reconstruct(x, seg)[0]
        model.ae.return_meshes = True        # (on the instance: the class default stays False)
        torch.manual_seed(4)
        wrapped = model.reconstruct(x, seg)[0]
        assert wrapped[2] is None and plain[2] is None
        for o in range(2):
            assert isinstance(wrapped[o], Meshes) and len(wrapped[o]) == 1
            verts = plain[o][0] if mode == 'accumulate' else plain[o][0].transpose(0, 1)
            assert torch.equal(wrapped[o].verts_padded()[0], verts), (mode, o)
            assert torch.equal(wrapped[o].faces_padded()[0].long(), model.ae.decoder.faces[0].long())


def test_forward_and_metrics(device, tmp_path):
    from fissure_segmentation_amd.dseg_ae_regularization import reconstruction_metrics
    model, _ = _models(tmp_path, True)
    model = model.to(device).eval()
    x, seg = _cloud(9, 1, device)
    torch.manual_seed(1)
    meshes, points, hidden = model(x, return_hidden=True)
    pred = model.segment(x)
    assert pred.shape == (1, N_CLOUD) and len(meshes) == len(points) == len(hidden) == 3
    for o in range(3):
        assert (meshes[o] is None) == (hidden[o] is None)
        assert meshes[o] is None or (meshes[o].shape == (1, 3, N_AE) and bool(torch.isfinite(meshes[o]).all()))
    # the metrics on the hand-made segmentation: object 3 is missing, and only it
    torch.manual_seed(2)
    meshes, points = model.reconstruct(x, seg)
    quad = (torch.tensor([[-1., -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], device=device),
            torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=device))
    inputs = [x[0, :3, seg[0] == o].transpose(0, 1) for o in (1, 2, 3)]
    res = reconstruction_metrics(meshes, points, inputs, [quad] * 3, faces=model.ae.decoder.faces[0])
    assert res["percent_missing"] == pytest.approx(100 / 3)
    for key in ("chamfer", "assd", "sdsd", "hd", "hd95"):
        assert torch.isnan(res[key]).tolist() == [False, False, True], key
        assert bool((res[key][:2] >= 0).all())
    # Chamfer by pytorch3d's rule, restated with torch.cdist in fp64
    v, p = meshes[0][0].transpose(0, 1).double().cpu(), inputs[0].double().cpu()
    d = torch.cdist(v, p) ** 2
    want = d.min(1)[0].mean() + d.min(0)[0].mean()
    assert abs(float(res["chamfer"][0]) - float(want)) <= 1e-5 * float(want)
    # a point-cloud output goes through the pseudo-symmetric distance
    gen = torch.Generator(device=device).manual_seed(3)
    res_p = reconstruction_metrics(meshes, points, inputs, [quad] * 3, n_samples=2000, generator=gen)
    assert torch.isnan(res_p["assd"]).tolist() == [False, False, True] and float(res_p["chamfer"][0]) == float(res["chamfer"][0])
