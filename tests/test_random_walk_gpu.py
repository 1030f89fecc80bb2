"""GPU tests of the matrix-free random walker (csrc/random_walk.hip) and the lobes-to-fissures launch against the fp64
restatement in tests/random_walk_oracle.py.

Yardstick for probabilities: the direct fp64 solve of the reference's system.  The error allowed is
max(16 * 2^-24, 10 * e_cpu32), e_cpu32 being the same statistic of the oracle's own fp32 conjugate gradients at the same
tolerance.  Every figure is printed (`RW_PARITY ...`, run with -s) before it is asserted; profiles/random_walk_parity.txt is
where the lines of a run on an MI355X belong (none had been made when these tests were written: DESIGN.md says so).

Iteration counts reported by the solver are the TRUE stopping iterates (the device records them), not multiples of
`check_every`: test_default_tolerance checks that they do not move with the host's cadence."""
import functools
import warnings

import numpy as np
import pytest
import torch

import random_walk_oracle as ro

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
CASES = {
    "small": dict(shape=(20, 24, 28), n_seeds=40, n_lobes=4, seed=1),
    "odd": dict(shape=(33, 30, 37), n_seeds=60, n_lobes=5, seed=2, island=True),      # no extent a multiple of 64 or 256
    "slab": dict(shape=(9, 65, 130), n_seeds=60, n_lobes=4, seed=3, radius=0.32),      # rows cross wave and workgroup borders
}


@functools.lru_cache(maxsize=None)
def reference(case, mode, tol=1e-6):
    """volume, blocks, direct solve, fp64 probabilities and the fp32 yardstick -- computed once, never modified"""
    vol = ro.make_volume(**CASES[case])
    im = (vol["labels"] != 0) if mode == "binary" else vol["im"]
    blk = ro.blocks(ro.laplacian(im, mode), vol["labels"], vol["mask"])
    X = ro.direct_solve(blk)
    X32, iters32 = ro.pcg_all(blk, tol, np.float32)
    e_cpu32 = float(np.abs(X32 - X).max())
    prob = ro.probabilities(blk, X, vol["labels"].shape)
    for a in (X, prob, vol["mask"], vol["labels"], vol["im"]):
        a.setflags(write=False)
    return dict(vol=vol, im=im, blk=blk, X=X, prob=prob, e_cpu32=e_cpu32, bar=max(FLOOR, 10 * e_cpu32), iters32=iters32)


def _dev(ref, device):
    vol = ref["vol"]
    return (torch.from_numpy(np.ascontiguousarray(ref["im"])).to(device), torch.from_numpy(vol["labels"]).to(device),
            torch.from_numpy(vol["mask"]).to(device))


@pytest.mark.parametrize("mode", ["binary", "intensity"])
@pytest.mark.parametrize("case", list(CASES))
def test_probabilities_against_direct_solve(device, case, mode):
    from fissure_segmentation_amd.data_processing import random_walk as rw
    ref = reference(case, mode)
    im, labels, mask = _dev(ref, device)
    prob = rw.random_walk(rw.compute_laplace_matrix(im, mode), labels, mask, tol=1e-6)
    assert prob.shape == (*labels.shape, ref["blk"]["K"]) and prob.dtype == torch.float32
    got = prob.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref["prob"]).max())
    print(f"RW_PARITY probabilities case={case} mode={mode} unknowns={ref['blk']['xu'].size} K={ref['blk']['K']} tol=1e-6 "
          f"max_abs_err={err:.3e} e_cpu32={ref['e_cpu32']:.3e} bar={ref['bar']:.3e} cpu32_iters={ref['iters32']}")
    m, lab = ref["vol"]["mask"], ref["vol"]["labels"]
    assert np.all(got[~m] == 0)
    seeds = m & (lab != 0)
    onehot = np.eye(ref["blk"]["K"])[lab[seeds] - 1]
    assert np.array_equal(got[seeds], onehot)
    assert err <= ref["bar"]


@pytest.mark.parametrize("case", list(CASES))
def test_fill_lobes_labels(device, case):
    from fissure_segmentation_amd.data_processing import find_lobes
    ref = reference(case, "binary")
    _, labels, mask = _dev(ref, device)
    filled = find_lobes.fill_lobes(labels, mask, tol=1e-6)
    assert filled.dtype == torch.int64 and filled.shape == labels.shape
    got = filled.cpu().numpy()
    want = ro.fill_lobes(ref["prob"], ref["vol"]["mask"])
    unknown = np.zeros(labels.numel(), bool)
    unknown[ref["blk"]["xu"]] = True
    unknown = unknown.reshape(labels.shape)
    ambiguous = unknown & (ro.top_two_gap(ref["prob"]) < 2 * ref["bar"])
    if CASES[case].get("island"):   # a mask component without a seed: all probabilities are 0 there (a tie by construction)
        island = np.zeros(labels.shape, bool)
        island[:2, :2, :3] = True
        assert np.all(got[island] == 1) and np.all(want[island] == 1)
        ambiguous &= ~island
    share = ambiguous.sum() / unknown.sum()
    wrong = int(((got != want) & ~ambiguous).sum())
    print(f"RW_PARITY labels case={case} unknowns={int(unknown.sum())} ambiguous_share={share:.5f} "
          f"disagree_outside_ambiguous={wrong} disagree_total={int((got != want).sum())}")
    assert share <= 0.02
    assert wrong == 0
    assert np.all(got[~ref["vol"]["mask"]] == 0)


@pytest.mark.parametrize("case", ["small", "odd"])
def test_default_tolerance(device, case):
    from fissure_segmentation_amd import functional as F
    ref = reference(case, "binary")
    im, labels, mask = _dev(ref, device)
    prob, info = F.random_walk_solve(im, labels, mask, "binary", return_info=True)
    K, xu = ref["blk"]["K"], ref["blk"]["xu"]
    X = prob.cpu().numpy().astype(np.float64).reshape(-1, K)[xu]
    res = ro.true_residuals(ref["blk"], X)
    iters = info["iterations"].cpu().numpy()
    print(f"RW_PARITY default_tol case={case} tol=1e-3 iterations={iters.tolist()} true_residual={np.round(res, 6).tolist()} "
          f"reported={np.round(info['relative_residual'].cpu().numpy(), 6).tolist()}")
    assert np.all(res <= 2e-3)
    assert np.all(iters > 0) and np.all(info["relative_residual"].cpu().numpy() <= 1e-3 * (1 + 1e-6))
    # the true stopping iterate: another host cadence changes neither the counts nor a bit of the result
    prob7, info7 = F.random_walk_solve(im, labels, mask, "binary", check_every=7, return_info=True)
    assert torch.equal(info7["iterations"], info["iterations"]) and torch.equal(prob7, prob)
    assert np.any(iters % 25 != 0) or np.any(iters % 7 != 0)


def test_batch_items_equal_their_own_runs_bit_for_bit(device):
    from fissure_segmentation_amd import functional as F
    a, b = reference("small", "binary")["vol"], ro.make_volume((20, 24, 28), 40, n_lobes=5, seed=11)
    labels = torch.from_numpy(np.stack([a["labels"], b["labels"]])).to(device)
    mask = torch.from_numpy(np.stack([a["mask"], b["mask"]])).to(device)
    im = labels != 0
    assert int(labels[0].max()) == 4 and int(labels[1].max()) == 5
    both, info = F.random_walk_solve(im, labels, mask, "binary", tol=1e-6, num_labels=5, return_info=True)
    again = F.random_walk_solve(im, labels, mask, "binary", tol=1e-6, num_labels=5)
    assert both.shape == (2, 20, 24, 28, 5) and torch.equal(both, again)
    assert int(info["iterations"][0, 4]) == 0 and torch.all(both[0, ..., 4] == 0)   # the unused label: solved by x = 0
    for i in range(2):
        alone, info1 = F.random_walk_solve(im[i], labels[i], mask[i], "binary", tol=1e-6, num_labels=5, return_info=True)
        assert torch.equal(alone, both[i]) and torch.equal(info1["iterations"], info["iterations"][i])
    four = F.random_walk_solve(im[0], labels[0], mask[0], "binary", tol=1e-6)
    assert four.shape[-1] == 4 and torch.equal(four, both[0, ..., :4])
    print(f"RW_PARITY batch iterations={info['iterations'].tolist()}")


@pytest.mark.parametrize("shape", [(1, 17, 19), (7, 1, 9), (6, 5, 1), (11, 13)])
@pytest.mark.parametrize("mode", ["binary", "intensity"])
def test_stencil_edges(device, shape, mode):
    """no mask (every face is touched), seeds on the border and in corners, singleton dimensions, a 2-d image"""
    from fissure_segmentation_amd import functional as F
    rng = np.random.default_rng(sum(shape))
    labels = np.zeros(shape, np.int64)
    labels.ravel()[0], labels.ravel()[-1] = 1, 2
    border = np.where((np.indices(shape) == 0).any(0).ravel())[0]
    labels.ravel()[rng.choice(border[1:-1], 4, replace=False)] = [3, 1, 2, 3]
    im = (rng.integers(0, 2, shape) if mode == "binary" else rng.standard_normal(shape) * 10).astype(np.float32)
    blk = ro.blocks(ro.laplacian(im, mode), labels)
    want = ro.probabilities(blk, ro.direct_solve(blk), shape)
    X32, _ = ro.pcg_all(blk, 1e-6, np.float32)
    bar = max(FLOOR, 10 * float(np.abs(X32 - ro.direct_solve(blk)).max()))
    got = F.random_walk_solve(torch.from_numpy(im).to(device), torch.from_numpy(labels).to(device), None, mode, tol=1e-6)
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"RW_PARITY edges shape={shape} mode={mode} max_abs_err={err:.3e} bar={bar:.3e}")
    assert got.shape == (*shape, 3) and err <= bar


@pytest.mark.parametrize("shape,n_lobes,batch", [((8, 9, 10), 4, 1), ((7, 9, 67), 5, 1), ((5, 6, 7), 5, 3), ((1, 1, 130), 4, 1)])
def test_lobes_to_fissures_labels(device, shape, n_lobes, batch):
    from fissure_segmentation_amd import functional as F
    rng = np.random.default_rng(n_lobes + shape[2])
    vols = rng.integers(0, n_lobes + 1, (batch, *shape))
    vols[:, 0, 0, :4] = [n_lobes, 1, 2, 3]   # every volume holds the largest label, and labels sit on the border
    want = np.stack([ro.fissures_from_lobes(v) for v in vols])
    t = torch.from_numpy(vols).to(device)
    got = F.lobes_to_fissures_labels(t if batch > 1 else t[0])
    assert got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
    assert want.max() == (3 if n_lobes == 5 else 2)
    with pytest.raises(ValueError, match="4 or 5 lobes"):
        F.lobes_to_fissures_labels(t.clamp(max=3))


def test_lobes_to_fissures_end_to_end(device):
    from fissure_segmentation_amd.data_processing import find_lobes
    ref = reference("odd", "binary")
    _, labels, mask = _dev(ref, device)
    fissures, filled = find_lobes.lobes_to_fissures(labels, mask, tol=1e-6)
    assert fissures.dtype == torch.uint8 and filled.dtype == torch.int64
    want_filled = ro.fill_lobes(ref["prob"], ref["vol"]["mask"])
    want = ro.fissures_from_lobes(want_filled)
    # a voxel is comparable if no voxel of its cross is ambiguous in the sense of test_fill_lobes_labels
    unknown = np.zeros(labels.numel(), bool)
    unknown[ref["blk"]["xu"]] = True
    amb = unknown.reshape(labels.shape) & (ro.top_two_gap(ref["prob"]) < 2 * ref["bar"])
    amb[:2, :2, :3] = False   # the seedless island is label 1 on both sides
    near = amb.copy()
    for ax in range(3):
        near |= np.roll(amb, 1, ax) | np.roll(amb, -1, ax)   # (wrap-around only excludes more)
    got = fissures.cpu().numpy()
    print(f"RW_PARITY end_to_end excluded={int(near.sum())} fissure_voxels={int((want > 0).sum())} "
          f"disagree={int(((got != want) & ~near).sum())}")
    assert np.array_equal(got[~near], want[~near]) and (want > 0).sum() > 100
    assert np.array_equal(filled.cpu().numpy()[~amb], want_filled[~amb])


def test_max_iter_warns(device):
    from fissure_segmentation_amd import functional as F
    ref = reference("small", "binary")
    im, labels, mask = _dev(ref, device)
    with pytest.warns(RuntimeWarning, match="max_iter = 3"):
        prob, info = F.random_walk_solve(im, labels, mask, "binary", tol=1e-6, max_iter=3, return_info=True)
    assert torch.all(info["iterations"] == 3) and torch.all(info["relative_residual"] > 1e-6)
    assert torch.isfinite(prob).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        F.random_walk_solve(im, labels, mask, "binary", tol=1e-3)


def test_workspace_too_small_is_an_error_code(device):
    from fissure_segmentation_amd import _lib
    from fissure_segmentation_amd.functional import _p, _stream
    B, K, D, H, W = 1, 4, 6, 7, 8
    need = _lib.lib.fsg_random_walk_workspace_bytes(B, K, D, H, W)
    ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=device)
    im = torch.zeros(D, H, W, dtype=torch.uint8, device=device)
    labels = torch.zeros(D, H, W, dtype=torch.int32, device=device)
    stop, rel = torch.empty(K, dtype=torch.int32, device=device), torch.empty(K, dtype=torch.float32, device=device)
    rc = _lib.lib.fsg_random_walk_prep(_p(im), 0, _p(labels), 1, None, B, K, D, H, W, _p(ws), need - 1, _p(stop), _p(rel), _stream())
    assert rc == 1 and b"workspace" in _lib.lib.fsg_last_error()
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("fsg_random_walk_iterate", _p(im), 0, B, K, D, H, W, 0, 1, 1e-3, _p(ws), 16, _p(stop), _p(rel), _stream())
