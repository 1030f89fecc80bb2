"""GPU tests of csrc/poisson_disk.hip through functional.sample_elimination, of Meshes.sample_points_poisson_disk and of
shape_model.point_cloud_registration.register_all.  The yardstick of the kernel is the bit-exact numpy restatement
(tests/poisson_disk_oracle.eliminate): `keep` and `order` must be EQUAL.  The compositions above the kernel are tested by the rule
of poisson_reconstruction: the result equals the public pieces called by hand, bit for bit.  Shapes are the smallest at which the
kernel takes another path.  When FSG_POISSON_PARITY names a file, a line per case is appended to it
(profiles/poisson_disk_parity.txt is such a record)."""
import os

import numpy as np
import pytest
import torch

import poisson_disk_oracle as po

pytestmark = pytest.mark.gpu
WAVE, WORKGROUP, COORD_LDS_MAX, MAX_M = 64, 1024, 8128, 16384   # csrc/poisson_disk.hip: kMaxThreads, kCoordLdsMax, kMaxM


def record(line):
    print(line)
    path = os.environ.get("FSG_POISSON_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _square(M, seed):
    """M uniform points of the unit square and radii that give a sample about 15 neighbours"""
    R = np.float32(np.sqrt(15 / (np.pi * M))) if M > 16 else np.float32(0.8)
    return po.unit_square(seed, M), R, np.float32(R / 4)


def _cases():
    """name -> (points, R, r_min, n_keep)"""
    c = {}
    c["M1"] = (*_square(1, 1), 1)
    c["M2_keep1"] = (*_square(2, 2), 1)
    c["M2_keep2"] = (*_square(2, 2), 2)
    c["M65_one_past_a_wave"] = (*_square(WAVE + 1, 3), 20)
    c["M1024_workgroup"] = (*_square(WORKGROUP, 4), 700)
    c["M1025_a_lane_owns_two"] = (*_square(WORKGROUP + 1, 5), 400)
    c["M193_keep1"] = (*_square(193, 6), 1)
    c["M193_keep_all"] = (*_square(193, 6), 193)
    c["M8128_coordinates_in_lds"] = (*_square(COORD_LDS_MAX, 7), COORD_LDS_MAX - 64)
    c["M8129_coordinates_in_global"] = (*_square(COORD_LDS_MAX + 1, 8), COORD_LDS_MAX + 1 - 64)
    c["M16384_largest"] = (*_square(MAX_M, 9), MAX_M - 64)
    c["duplicates_and_pairs_below_r_min"] = (*po.duplicates_cloud(), 30)
    c["lattice_ties"] = (*po.lattice(), 60)
    p80 = po.unit_square(4, 80)
    c["no_neighbour_tiny_R"] = (p80, np.float32(1e-6), np.float32(0), 30)
    c["no_neighbour_R_zero"] = (p80, np.float32(0), np.float32(0), 30)
    c["no_neighbour_R_negative"] = (p80, np.float32(-1), np.float32(0.1), 30)
    return c


CASES = _cases()


def _run(device, points, R, r_min, n_keep, **kw):
    from fissure_segmentation_amd import functional as F_hip
    t = torch.from_numpy(np.ascontiguousarray(points)).to(device)
    before = t.clone()
    keep, order = F_hip.sample_elimination(t, n_keep, R, r_min, return_order=True, **kw)
    assert torch.equal(t, before) and keep.dtype == order.dtype == torch.int64
    return keep.cpu().numpy(), order.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement(device, name):
    p, R, r_min, n_keep = CASES[name]
    want_keep, want_order = po.eliminate(p, n_keep, R, r_min)
    keep, order = _run(device, p, float(R), float(r_min), n_keep)
    same = np.array_equal(keep, want_keep) and np.array_equal(order, want_order)
    first = int(np.argmax(order != want_order)) if order.shape == want_order.shape and not np.array_equal(order, want_order) else -1
    record(f"{name}: M={len(p)} n_keep={n_keep} R={float(R):.6g} r_min={float(r_min):.6g} keep and order "
           f"{'equal' if same else 'DIFFER'} (first differing round {first})")
    assert keep.shape == (n_keep,) and order.shape == (len(p) - n_keep,)
    assert np.array_equal(order, want_order) and np.array_equal(keep, want_keep)


def test_batch_items_equal_their_solo_runs_repeat_and_replay(device):
    """B = 3 items with different R and r_min, given as device tensors: every item equals its solo run and the restatement, a
    second run gives the same bits, and so does a replay of the call captured in a graph"""
    from fissure_segmentation_amd import functional as F_hip
    M, n_keep = 321, 100
    pts = np.stack([po.unit_square(20 + b, M) for b in range(3)])
    R = np.array([0.12, 0.05, 0.3], np.float32)
    r_min = np.array([0.03, 0.0, 0.1], np.float32)
    t, Rt, rt = (torch.from_numpy(a).to(device) for a in (pts, R, r_min))
    keep, order = F_hip.sample_elimination(t, n_keep, Rt, rt, return_order=True)
    assert keep.shape == (3, n_keep) and order.shape == (3, M - n_keep)
    for b in range(3):
        want = po.eliminate(pts[b], n_keep, R[b], r_min[b])
        assert np.array_equal(keep[b].cpu().numpy(), want[0]) and np.array_equal(order[b].cpu().numpy(), want[1])
        alone = F_hip.sample_elimination(t[b], n_keep, float(R[b]), float(r_min[b]), return_order=True)
        assert alone[0].shape == (n_keep,) and torch.equal(alone[0], keep[b]) and torch.equal(alone[1], order[b])
    again = F_hip.sample_elimination(t, n_keep, Rt, rt, return_order=True)
    assert torch.equal(again[0], keep) and torch.equal(again[1], order)
    assert torch.equal(F_hip.sample_elimination(t, n_keep, Rt, rt), keep)            # without the order
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph):
            cap = F_hip.sample_elimination(t, n_keep, Rt, rt, return_order=True)
    torch.cuda.current_stream().wait_stream(side)
    cap[0].zero_()
    cap[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap[0], keep) and torch.equal(cap[1], order)


# ------------------------------------------------------------------ mesh level
def _test_meshes(device):
    from fissure_segmentation_amd.mesh import Meshes
    square = (np.array([[0., 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]]))
    octa = (np.array([[1.5, 0, 0], [-1.5, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float32),
            np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))
    arrays = [square, octa]
    return arrays, Meshes([torch.from_numpy(v).to(device) for v, _ in arrays], [torch.from_numpy(f).to(device) for _, f in arrays])


@pytest.mark.parametrize("N,init_factor", [(50, 5), (37, 3), (40, 1)])
def test_mesh_sampler_equals_its_composition_by_hand(device, N, init_factor):
    """a two-triangle square and a closed octahedron in one batch: same uniforms -> sample_points_from_uniforms -> open3d's
    radii from the fp64 area -> oracle elimination -> gather"""
    import mesh_oracle
    from fissure_segmentation_amd import mesh as M_hip
    arrays, meshes = _test_meshes(device)
    M = init_factor * N
    gen = torch.Generator(device=device).manual_seed(123)
    got, rows = meshes.sample_points_poisson_disk(N, init_factor=init_factor, generator=gen, return_indices=True)
    assert got.shape == (2, N, 3) and got.dtype == torch.float32 and rows.shape == (2, N) and not got.requires_grad
    gen = torch.Generator(device=device).manual_seed(123)
    u = torch.rand(2, M, 3, device=device, dtype=torch.float32, generator=gen)
    pts = M_hip.sample_points_from_uniforms(meshes, u).cpu().numpy()
    for b, (v, f) in enumerate(arrays):
        area = float(mesh_oracle.face_cdf(torch.from_numpy(v), torch.from_numpy(f))[-1])
        R, r_min = po.radii(area, N, M)
        keep, _ = po.eliminate(pts[b], N, R, r_min)
        assert np.array_equal(rows[b].cpu().numpy(), keep)
        assert np.array_equal(got[b].cpu().numpy().view(np.uint32), pts[b][keep].view(np.uint32))
        if init_factor == 5:
            ratio = po.min_nn_distance(pts[b][keep]) / R
            record(f"mesh {b} N={N} of M={M}: area {area:.6g} R={float(R):.6g}, min nearest-neighbour distance / R = {ratio:.3f} "
                   f"(first N uniform samples: {po.min_nn_distance(pts[b][:N]) / R:.3f})")
    if init_factor == 1:
        assert np.array_equal(rows.cpu().numpy(), np.tile(np.arange(N), (2, 1)))
    # the module-level form, and the same seed gives the same bits
    gen = torch.Generator(device=device).manual_seed(123)
    assert torch.equal(M_hip.sample_points_poisson_disk(meshes, N, init_factor=init_factor, generator=gen), got)


# ------------------------------------------------------------------ the registration driver
def test_evaluate_registration_equals_brute_force(device):
    from fissure_segmentation_amd.shape_model.point_cloud_registration import evaluate_registration
    rng = np.random.default_rng(0)
    src, tgt = rng.random((2, 70, 3)), rng.random((2, 90, 3))
    nn = np.sqrt(((src[:, :, None].astype(np.float32) - tgt[:, None].astype(np.float32)).astype(np.float64) ** 2).sum(-1)).min(-1)
    # a limit in the middle of the widest gap of the sorted distances around the median: no point sits near the threshold
    limits = []
    for b in range(2):
        s = np.sort(nn[b])[20:50]
        k = int(np.argmax(np.diff(s)))
        limits.append(0.5 * (s[k] + s[k + 1]))
    limits = np.array(limits)
    out = evaluate_registration(src, tgt, limits)
    inl = nn <= limits[:, None]
    assert np.array_equal(out["n_correspondences"], inl.sum(1)) and np.array_equal(out["fitness"], inl.sum(1) / 70)
    np.testing.assert_allclose(out["inlier_rmse"], np.sqrt((nn ** 2 * inl).sum(1) / inl.sum(1)), rtol=1e-6)
    one = evaluate_registration(src[0], tgt[0], float(limits[0]))
    assert one["n_correspondences"] == inl[0].sum() and isinstance(one["fitness"], float)
    t = evaluate_registration(torch.from_numpy(src).to(device), torch.from_numpy(tgt).to(device), torch.from_numpy(limits).to(device))
    assert t["n_correspondences"].is_cuda and np.array_equal(t["n_correspondences"].cpu().numpy(), inl.sum(1))
    none = evaluate_registration(src, tgt + 10, 0.5)
    assert not none["n_correspondences"].any() and not none["inlier_rmse"].any()
    tie = evaluate_registration(np.zeros((1, 3)), np.array([[3., 4, 0]]), 5.0)        # <=: a point AT the distance counts
    assert tie["n_correspondences"] == 1 and tie["inlier_rmse"] == 5.0


def test_register_all_is_its_public_pieces_and_feeds_the_shape_model(device):
    from fissure_segmentation_amd.mesh import Meshes
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    from fissure_segmentation_amd.shape_model.generate_corresponding_points import data_set_correspondences
    from fissure_segmentation_amd.shape_model.ssm import SSM
    I, O, P, M = po.REG_INSTANCES, po.REG_OBJECTS, po.REG_POINTS, po.REG_INIT_FACTOR * po.REG_POINTS
    fixed, meshes = po.fixed_clouds(), po.moving_surfaces()
    ids = [("case%d" % i, "fixed") for i in range(I)]
    gen = torch.Generator(device=device).manual_seed(7)
    out = pcr.register_all(list(fixed), meshes, ids, "unused", generator=gen, pair_batch=4)
    for k in ("displacements", "moved_pcs", "moving_pcs"):
        assert isinstance(out[k], np.ndarray) and out[k].shape == (I, O, P, 3) and out[k].dtype == np.float64
    assert out["n_correspondences"].shape == out["corr_distances"].shape == (I, O) and out["ids"].shape == (I, 2)
    assert len(out["transforms"]) == I and set(out["transforms"][0]) == {"scale", "translation", "rotation"}

    # ---- the public pieces by hand, same generator state, same batches: bit for bit
    gen = torch.Generator(device=device).manual_seed(7)
    uniforms, moving = [], []
    for o in range(O):
        state = gen.get_state()
        uniforms.append(torch.rand(I, M, 3, device=device, dtype=torch.float32, generator=gen).cpu().numpy())
        gen.set_state(state)
        batch = Meshes([torch.from_numpy(meshes[i][o][0]).to(device) for i in range(I)],
                       [torch.from_numpy(meshes[i][o][1]).to(device) for i in range(I)])
        moving.append(batch.sample_points_poisson_disk(P, generator=gen))
    moving = torch.stack(moving, 1).double()
    fx = torch.from_numpy(fixed).to(device)
    prereg, (s, rot, t) = pcr.RigidRegistration(X=fx.reshape(O * P, 3), Y=moving.reshape(I, O * P, 3)).register()
    X, Y = fx[None].expand(I, O, P, 3).reshape(I * O, P, 3), prereg.reshape(I * O, P, 3)
    first, second = pcr.register_cpd_deformable(X[:4].contiguous(), Y[:4].contiguous()), \
        pcr.register_cpd_deformable(X[4:].contiguous(), Y[4:].contiguous())
    moved, disp = torch.cat([first[0], second[0]]), torch.cat([first[1], second[1]])
    heur = pcr.correspondence_distance_heuristic(fx)
    found = pcr.evaluate_registration(moved.float(), X.float(), heur[None].expand(I, O).reshape(-1))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)   # noqa: E731
    assert np.array_equal(bits(out["moving_pcs"]), bits(moving.cpu().numpy()))
    assert np.array_equal(bits(out["moved_pcs"]), bits(moved.reshape(I, O, P, 3).cpu().numpy()))
    assert np.array_equal(bits(out["displacements"]), bits(disp.reshape(I, O, P, 3).cpu().numpy()))
    assert np.array_equal(out["n_correspondences"], found["n_correspondences"].reshape(I, O).cpu().numpy())
    assert np.array_equal(bits(out["corr_distances"]), bits(heur[None].expand(I, O).cpu().numpy()))
    for i, tr in enumerate(out["transforms"]):
        assert tr["scale"] == float(s[i]) and np.array_equal(tr["translation"], t[i].cpu().numpy())
        assert np.array_equal(tr["rotation"], rot[i].T.cpu().numpy())        # transposed: A x instead of x A
        np.testing.assert_allclose(tr["scale"] * out["moving_pcs"][i].reshape(-1, 3) @ tr["rotation"].T + tr["translation"],
                                   prereg[i].cpu().numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["moved_pcs"] - out["displacements"], prereg.reshape(I, O, P, 3).cpu().numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["corr_distances"][0], [pcr.correspondence_distance_heuristic(f) for f in fixed], rtol=1e-14)

    # ---- the same pipeline on the CPU from the oracles, on the same uniforms: every registered point lies within half the
    # heuristic distance of its fixed cloud, so every point is a correspondence, here and there
    cpu = po.register_all_cpu(fixed, meshes, uniforms)
    gpu_nn = np.sqrt(((out["moved_pcs"][:, :, :, None] - fixed[None, :, None]) ** 2).sum(-1)).min(-1)
    record(f"register_all {I} x {O} x {P}: largest distance of a registered point to its fixed cloud: CPU oracles "
           f"{cpu['nn'].max():.4f}, GPU {gpu_nn.max():.4f}; heuristic distances {cpu['heuristic']}; largest difference of the "
           f"sampled clouds {np.abs(cpu['moving'] - out['moving_pcs']).max():.3e}, of the registered clouds "
           f"{np.abs(cpu['moved'] - out['moved_pcs']).max():.3e}")
    assert (cpu["nn"] <= 0.5 * cpu["heuristic"][None, :, None]).all()
    assert np.array_equal(out["n_correspondences"], np.full((I, O), P))
    rows = out["correspondences"]
    assert rows["Object No."] == ["1", "2", "mean"] and rows["Mean corresponding"] == [1.0, 1.0, 1.0]
    assert rows["StdDev corresponding"] == [0.0, 0.0, 0.0]
    np.testing.assert_allclose(rows["Max. corr dist"], list(cpu["heuristic"]) + [cpu["heuristic"].mean()], rtol=1e-12)

    # ---- the outputs feed data_set_correspondences and SSM.fit unchanged
    pcs, transforms, fixed_pc, labels, evaluation = data_set_correspondences(
        fixed, meshes, out["moving_pcs"], out["transforms"], out["moved_pcs"], out["displacements"], mode="simple", show=False)
    assert pcs.shape == (I, O * P, 3) and fixed_pc.shape == (O * P, 3) and labels.tolist() == [1] * P + [2] * P
    assert all(np.isfinite(np.asarray(v)).all() for v in evaluation.values()) and np.isfinite(pcs).all()
    record(f"register_all -> data_set_correspondences(simple): mean distance of the corresponding points to the instances' "
           f"meshes {np.asarray(evaluation['mean']).max():.4f} at most")
    ssm = SSM().to(device)
    ssm.fit(torch.from_numpy(pcs).float().to(device))
    assert 1 <= int(ssm.num_modes) <= I and torch.isfinite(ssm.eigenvectors).all() and ssm.mean_shape.shape == (1, O * P * 3)

    # ---- GPU tensors in, GPU tensors out, same bits
    gen = torch.Generator(device=device).manual_seed(7)
    dev_out = pcr.register_all(fx, meshes, generator=gen, pair_batch=4)
    assert dev_out["moved_pcs"].is_cuda and dev_out["ids"].tolist() == [0, 1, 2] and dev_out["transforms"][0]["rotation"].is_cuda
    for k in ("displacements", "moved_pcs", "moving_pcs", "n_correspondences", "corr_distances"):
        assert np.array_equal(dev_out[k].cpu().numpy(), out[k])
