"""GPU tests of csrc/kmeans.hip through functional.kmeans_step / functional.kmeans.  The yardstick is the bit-exact numpy
restatement of the kernel (tests/kmeans_oracle.Restatement): labels, counts, centres, inertia and the number of changed labels
must be EQUAL, bit for bit; the fp64 Lloyd of the same file bounds what the fp32 distances may cost.  Measured figures are printed
and, when FSG_KMEANS_PARITY names a file, appended to it (profiles/kmeans_parity.txt is such a record)."""
import os

import numpy as np
import pytest
import torch

import kmeans_oracle as ko

pytestmark = pytest.mark.gpu
TILE, CHUNK = 256, 1024   # csrc/kmeans.hip: kThreads (points of a workgroup's tile), kChunk (centres staged at once)
HOUSE_BAR = 4.8e-7


def record(line):
    print(line)
    path = os.environ.get("FSG_KMEANS_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _cloud(n, seed, offset=0., scale=1.):
    rng = np.random.default_rng(seed)
    return (scale * np.stack([60 * rng.uniform(-1, 1, n), 45 * rng.uniform(-1, 1, n), 12 * rng.standard_normal(n)], 1)
            + offset).astype(np.float32)


def _pick(pts, K, seed):
    return pts[np.random.default_rng(seed).choice(len(pts), K, replace=False)].copy()


def _step_cases():
    """name -> list of items (points (n,3), centres (K,3), previous labels or None); the items of a case share n and K"""
    cases = {}
    a, b = _cloud(193, 1), _cloud(193, 2)
    cases["B2_n193_K37"] = [(a, _pick(a, 37, 3), None), (b, _pick(b, 37, 4), None)]            # partial wave, partial tile
    cases["n1_K1"] = [(_cloud(1, 5), _cloud(1, 6), None)]
    cases["K1"] = [(a, a[:1] + 1, None)]
    p70 = _cloud(70, 7)
    cases["K_equals_n_70"] = [(p70, p70.copy(), None)]                                            # inertia exactly 0
    big = _cloud(1100, 8)
    cases["K1025_n1100"] = [(big, _pick(big, CHUNK + 1, 9), None)]                                # one more than a staged chunk
    # the LDS accumulators (28 K bytes) beside the 16 KiB centre tile: K = 1756 is the first size that needs more than the
    # 64 KiB a kernel gets unasked; K = 4096 is the largest the kernel serves (four staged chunks)
    wide = _cloud(4200, 24)
    cases["K1756_n1800"] = [(wide[:1800], _pick(wide[:1800], 1756, 25), None)]
    cases["K4096_n4200"] = [(wide, _pick(wide, 4096, 26), None), (wide[::-1].copy(), _pick(wide, 4096, 27), None)]
    one_more = _cloud(TILE + 1, 10)
    cases["n_tile_plus_1"] = [(one_more, _pick(one_more, 11, 11), None)]
    spread = _cloud(2 * 2048 * TILE // 8 + 3, 12)                                                 # more tiles than workgroups: a
    cases["several_tiles_per_workgroup"] = [(spread, _pick(spread, 5, 13), None)] * 8             # workgroup walks 2 tiles (B = 8)
    co = _pick(a, 9, 14)
    co[6] = co[2]
    cases["coincident_centres"] = [(a, co, None)]
    dup = np.concatenate([a[:50], a[:50], a[:50], a[50:93]])                                      # 193 rows, 100 of them repeats
    cases["duplicated_points"] = [(dup, _pick(a[:93], 13, 15), None)]
    off = _cloud(193, 16, offset=500.)
    cases["offset_500"] = [(off, _pick(off, 37, 17), None)]
    tiny, huge = _cloud(193, 18, scale=1e-3), _cloud(193, 19, scale=1e3)
    cases["mixed_scales"] = [(tiny, _pick(tiny, 37, 20), None), (a, _pick(a, 37, 21), None), (huge, _pick(huge, 37, 22), None)]
    prev = np.random.default_rng(23).integers(0, 37, 193).astype(np.int32)
    cases["previous_labels"] = [(a, _pick(a, 37, 3), prev), (b, _pick(b, 37, 4), prev[::-1].copy())]
    return cases


STEP_CASES = _step_cases()


def _gpu_step(items, device):
    from fissure_segmentation_amd import functional as F_hip
    pts = torch.from_numpy(np.stack([it[0] for it in items])).to(device)
    cen = torch.from_numpy(np.stack([it[1] for it in items])).to(device)
    prev = None if items[0][2] is None else torch.from_numpy(np.stack([it[2] for it in items])).to(device)
    keep = (pts.clone(), cen.clone())
    out = F_hip.kmeans_step(pts, cen, prev)
    assert torch.equal(pts, keep[0]) and torch.equal(cen, keep[1])     # the inputs are not modified
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[2].dtype == torch.int32
    assert out[3].dtype == torch.float64 and out[4].dtype == torch.int32
    return [t.cpu().numpy() for t in out]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_equals_the_restatement_bit_for_bit(device, name):
    items = STEP_CASES[name]
    labels, centres, counts, inertia, changed = _gpu_step(items, device)
    done = {}
    for b, (p, c, prev) in enumerate(items):
        r = done.get(id(p))                        # (the items of one case that are the same arrays share their restatement)
        if r is None:
            r = done[id(p)] = ko.Restatement(p, c, prev_labels=prev)
            r.step()
        assert np.array_equal(labels[b], r.labels), (name, b, int((labels[b] != r.labels).sum()))
        assert np.array_equal(counts[b], r.counts) and int(changed[b]) == r.n_changed
        assert np.array_equal(_bits(centres[b]), _bits(r.c)), (name, b, np.abs(centres[b] - r.c).max())
        assert float(inertia[b]) == r.inertia, (name, b, float(inertia[b]), r.inertia)
    if name == "K_equals_n_70":
        assert float(inertia[0]) == 0. and np.array_equal(labels[0], np.arange(70)) and np.array_equal(_bits(centres[0]), _bits(items[0][1]))
    if name == "coincident_centres":
        assert counts[0][6] == 0 and counts[0][2] > 0 and np.array_equal(_bits(centres[0][6]), _bits(items[0][1][6]))
    if name == "previous_labels":
        assert 0 < int(changed[0]) < 193


@pytest.mark.parametrize("size", ["12x37", "20x256"])
def test_step_labels_against_the_fp64_oracle(device, size):
    """labels equal the fp64 oracle's except where its two best squared distances differ by less than 1e-5 relative (about forty
    times the fp32 rounding of the direct form); at most 0.1 % of the points may be excused that way"""
    I, P = (12, 37) if size == "12x37" else (20, 256)
    pts = ko.pooled(I, P, 5)
    for what, c in (("initial", pts[ko.fps32(pts, P)]), ("converged", ko.run(pts, pts[ko.fps32(pts, P)])["centres"])):
        labels = _gpu_step([(pts, c, None)], device)[0][0]
        lab, best, second = ko.assign64(pts, c)
        excused = (second - best) < 1e-5 * second
        record(f"kmeans step {size} {what} centres: {int(excused.sum())} of {len(pts)} points excused, "
               f"{int((labels != lab).sum())} labels differ from fp64")
        assert excused.mean() <= 1e-3 and np.array_equal(labels[~excused], lab[~excused])


@pytest.fixture(scope="module")
def whole_runs(device):
    """size -> (points (B,n,3), first centres (B,K,3) from the package's own farthest point sampling, the kmeans outputs)"""
    from fissure_segmentation_amd import functional as F_hip
    out = {}
    for size, (B, I, P) in {"B2_12x37": (2, 12, 37), "B1_20x256": (1, 20, 256)}.items():
        pts = torch.from_numpy(np.stack([ko.pooled(I, P, 5 + b) for b in range(B)])).to(device)
        seg = torch.arange(1, B + 1, dtype=torch.int32, device=device)
        rows = F_hip.fps(pts.reshape(-1, 3), seg * I * P, seg * P, B * P).long().view(B, P) - (seg.long() - 1)[:, None] * I * P
        c0 = torch.gather(pts, 1, rows[:, :, None].expand(B, P, 3)).contiguous()
        out[size] = (pts, c0, F_hip.kmeans(pts, P, init='fps', return_info=True))
    return out


@pytest.mark.parametrize("size", ["B2_12x37", "B1_20x256"])
def test_whole_run_equals_the_restatement(device, whole_runs, size):
    from fissure_segmentation_amd import functional as F_hip
    pts, c0, (cen, lab, inertia, n_iter, info) = whole_runs[size]
    B, n, K = pts.shape[0], pts.shape[1], c0.shape[1]
    assert cen.shape == (B, K, 3) and cen.dtype == torch.float32 and lab.shape == (B, n) and lab.dtype == torch.int64
    assert inertia.shape == (B,) and inertia.dtype == torch.float64 and n_iter.shape == (B,)
    for b in range(B):
        p, c = pts[b].cpu().numpy(), c0[b].cpu().numpy()
        r = ko.run(p, c)
        assert int(n_iter[b]) == r["n_iter"] and 2 < r["n_iter"] < 300
        assert np.array_equal(_bits(cen[b].cpu().numpy()), _bits(r["centres"]))
        assert np.array_equal(lab[b].cpu().numpy(), r["labels"]) and float(inertia[b]) == r["inertia"]
        assert np.array_equal(info["counts"][b].cpu().numpy(), r["counts"]) and int(info["n_empty"][b]) == r["n_empty"]
        # quality: below the inertia of the first centres; equal to the fp64 Lloyd's from the same centres to within 4 x the
        # restatement's own deviation from it (floor: the house bar)
        o = ko.lloyd64(p, c)
        dev_restatement = abs(r["inertia"] - o["inertia"]) / o["inertia"]
        dev_kernel = abs(float(inertia[b]) - o["inertia"]) / o["inertia"]
        record(f"kmeans run {size} item {b}: {r['n_iter']} iterations, inertia {float(inertia[b]):.6f} (first centres "
               f"{r['inertias'][0]:.6f}), fp64 Lloyd {o['inertia']:.6f}, relative deviation kernel {dev_kernel:.3e} "
               f"restatement {dev_restatement:.3e}")
        assert float(inertia[b]) < r["inertias"][0]
        assert dev_kernel <= max(4 * dev_restatement, HOUSE_BAR)
    # an explicit init with the same rows gives the same bits; so does a second run; so does an item on its own
    again = F_hip.kmeans(pts, init=c0)
    second = F_hip.kmeans(pts, K, init='fps')
    for x, y, z in zip((cen, lab, inertia, n_iter), again, second):
        assert torch.equal(x, y) and torch.equal(x, z)
    alone = F_hip.kmeans(pts[B - 1], K)
    assert alone[0].shape == (K, 3) and alone[1].shape == (n,) and alone[2].dim() == 0 and alone[3].dim() == 0
    for x, y in zip((cen, lab, inertia, n_iter), alone):
        assert torch.equal(x[B - 1], y)


def test_inertia_never_increases_and_max_iter(device, whole_runs):
    from fissure_segmentation_amd import functional as F_hip
    pts, c0, (cen, lab, inertia, n_iter, _) = whole_runs["B2_12x37"]
    c, prev, series = c0, None, []
    for _ in range(int(n_iter.max())):
        prev, c, _, val, _ = F_hip.kmeans_step(pts, c, prev)
        series.append(val.cpu().numpy())
    series = np.stack(series)
    assert (series[1:] <= series[:-1]).all() and (inertia.cpu().numpy() <= series[-1]).all()
    one = F_hip.kmeans(pts, init=c0, max_iter=1)
    assert one[3].tolist() == [1, 1]
    first = F_hip.kmeans_step(pts, c0)
    assert torch.equal(one[0], first[1])
    zero = F_hip.kmeans(pts, init=c0, max_iter=0)
    assert zero[3].tolist() == [0, 0] and torch.equal(zero[0], c0) and torch.equal(zero[1], first[0].long())
    assert torch.equal(zero[2], first[3])


def test_a_converged_item_is_frozen_beside_an_unconverged_one(device, whole_runs):
    from fissure_segmentation_amd import functional as F_hip
    """tol = 0: a run ends at a fixed point (no label changes).  Started there, an item stops after its first iteration -- all
    labels are new to it, but the sums and so the centres are the same bits, shift 0 -- and must stay as it is while the other
    item of the batch runs on"""
    pts, c0, _ = whole_runs["B2_12x37"]
    cen, lab, inertia, n_iter = F_hip.kmeans(pts, init=c0, tol=0.)
    mixed = torch.stack([cen[0], c0[1]])          # item 0 starts at its converged centres, item 1 at the first ones
    out = F_hip.kmeans(pts, init=mixed, tol=0.)
    assert int(out[3][0]) == 1 and int(out[3][1]) == int(n_iter[1]) > 1
    assert torch.equal(out[0][0], cen[0]) and torch.equal(out[1][0], lab[0]) and torch.equal(out[2][0], inertia[0])
    assert torch.equal(out[0][1], cen[1]) and torch.equal(out[1][1], lab[1]) and torch.equal(out[2][1], inertia[1])


def test_record_quality_against_sklearn(device, whole_runs):
    """records, asserts nothing: final inertia over that of sklearn's k_means (k-means++, n_init = 1, five seeds)"""
    cluster = pytest.importorskip("sklearn.cluster")
    for size in ("B2_12x37", "B1_20x256"):
        pts, c0, (cen, lab, inertia, n_iter, _) = whole_runs[size]
        p = pts[0].cpu().numpy().astype(np.float64)
        theirs = [cluster.k_means(p, n_clusters=c0.shape[1], random_state=s, n_init=1)[2] for s in range(5)]
        record(f"kmeans quality {size} item 0: inertia {float(inertia[0]):.1f}, sklearn over five seeds {min(theirs):.1f} .. "
               f"{max(theirs):.1f}, ratio to their mean {float(inertia[0]) / np.mean(theirs):.4f}")
