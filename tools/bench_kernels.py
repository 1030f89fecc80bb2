"""Micro-benchmark of single C-ABI entry points (HIP-event timed, median of many launches)."""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fissure_segmentation_amd as fsg
from golden_util import cloud
F = fsg.functional
dev = torch.device("cuda:0")


def timeit(fn, iters=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ts), min(ts)


which = sys.argv[1:] or ["knn"]
if "knn" in which:
    for (B, C, N, k) in [(8, 3, 2048, 20), (8, 64, 2048, 20), (4, 3, 8192, 40), (4, 64, 8192, 40), (8, 128, 2048, 20), (8, 64, 4096, 20),
                         (8, 128, 4096, 20), (8, 3, 4096, 20)]:
        x = torch.from_numpy(cloud(1, B, C, N)).to(dev)
        for name, rows, dbg in (("split (default)", False, 0), ("two-phase", False, fsg._lib.KNN_DBG_TWO_PHASE),
                                ("mfma(v1)", False, fsg._lib.KNN_FORCE_MFMA), ("rows(v0)", True, 0)):
            med, mn = timeit(lambda: F.knn_graph(x, k, force_rows_kernel=rows, _debug_flags=dbg))
            print(f"knn B={B} C={C} N={N} k={k} {name:15s}: median {med:8.1f} us  min {mn:8.1f} us")
if "edgeconv" in which:
    from fissure_segmentation_amd.models.dgcnn import EdgeConv
    for (B, C, N, k, couts) in [(8, 64, 2048, 20, [64]), (8, 3, 2048, 20, [64, 64]), (4, 64, 8192, 40, [64]), (4, 3, 8192, 40, [64, 64])]:
        ec = EdgeConv(C, couts, k, first_layer=(C == 3)).to(dev).train()
        x = torch.from_numpy(cloud(1, B, C, N)).to(dev).requires_grad_(True)
        idx = F.knn_graph(x, k, c_knn=3 if C == 3 else None)
        g = torch.randn(B, couts[-1], N, device=dev)
        med, mn = timeit(lambda: ec(x, idx))
        print(f"edgeconv fwd B={B} C={C} N={N} k={k} {couts}: median {med:8.1f} us min {mn:8.1f}")
        def fb():
            y = ec(x, idx); y.backward(g)
        med, mn = timeit(fb)
        print(f"edgeconv fwd+bwd                          : median {med:8.1f} us min {mn:8.1f}")
if "ec2" in which:
    from fissure_segmentation_amd.models.dgcnn import EdgeConv
    B, C, N, k = 8, 3, 2048, 20
    ec = EdgeConv(C, [64, 64], k, first_layer=True).to(dev).train()
    x = torch.from_numpy(cloud(1, B, C, N)).to(dev).requires_grad_(True)
    idx = F.knn_graph(x, k, c_knn=3)
    g = torch.randn(B, 64, N, device=dev)
    def fb():
        y = ec(x, idx); y.backward(g)
    fsg._lib.start_timing()
    for _ in range(20): fb()
    ms = fsg._lib.stop_timing()
    for n, v in ms.items():
        v = sorted(v)[len(v)//2]
        print(f"  {n}: median {1e3*v:.1f} us")
if "chamfer" in which:
    for (B, N) in [(8, 2048), (8, 4096)]:
        a = torch.rand(B, N, 3, device=dev); b = torch.rand(B, N, 3, device=dev)
        med, mn = timeit(lambda: F.chamfer_nn(a, b))
        print(f"chamfer_nn B={B} N={N}: median {med:8.1f} us min {mn:8.1f}")
if "ssmdec" in which:   # DG-SSM's decode + similarity transform: fused stage vs the torch composition of the same math
    from fissure_segmentation_amd.augmentations import so3_exp_map
    for (B, P, M) in [(32, 2048, 20), (32, 2048, 32), (4, 4097, 64)]:
        mean, evec = torch.rand(3 * P, device=dev) * 2 - 1, torch.randn(3 * P, M, device=dev) / M ** 0.5
        w, v, s, tr = (t.requires_grad_(True) for t in (torch.randn(B, M, device=dev), 0.5 * torch.randn(B, 3, device=dev),
                                                        torch.rand(B, 3, device=dev) + 0.5, torch.randn(B, 3, device=dev)))
        g = torch.randn(B, P, 3, device=dev)

        def torch_form():   # SSM.decode + compose_transform + transform_points without the 4x4 detour (fewer launches than the reference)
            x = (mean[None] + torch.matmul(evec[None], w[:, :, None]).squeeze(-1)).unflatten(-1, (P, 3))
            return torch.bmm(x, so3_exp_map(v)) * s[:, None, :] + tr[:, None, :]
        for name, fn in (("fused fsg_ssm_decode", lambda: F.ssm_decode_affine(w, mean, evec, v, s, tr)), ("torch composition", torch_form)):
            med_f, min_f = timeit(fn, iters=100, warm=10)
            out = fn()
            med_b, min_b = timeit(lambda: torch.autograd.grad(out, (w, v, s, tr), g, retain_graph=True), iters=100, warm=10)
            print(f"ssmdec B={B} P={P} M={M} {name:22s}: fwd median {med_f:7.1f} us (min {min_f:7.1f})  "
                  f"bwd median {med_b:7.1f} us (min {min_b:7.1f})")
if "maxavg" in which:   # conv5's BatchNorm + LeakyReLU + [max | mean] pooling at the DG-SSM shape: fused vs torch composition
    from fissure_segmentation_amd.norm import BatchNorm1d
    B, N, C = 32, 1024, 1024
    nbytes = B * N * C * 4
    bn = BatchNorm1d(C).to(dev).train()
    y = torch.randn(B, N, C, device=dev).requires_grad_(True)
    g = torch.randn(B, 2 * C, device=dev)

    def torch_form(y):
        a = torch.nn.functional.leaky_relu(bn(y.view(B * N, C)), 0.2).view(B, N, C)
        return torch.cat((a.max(dim=1)[0], a.mean(dim=1)), 1)
    for name, fn, fwd_bytes, bwd_bytes in (("fused fsg_bn_act_maxavg", lambda y: F.bn_act_maxavg(y, bn, 0.2), 2 * nbytes, 3 * nbytes),
                                           ("torch BN+LeakyReLU+max+mean", torch_form, None, None)):
        med_f, _ = timeit(lambda: fn(y))
        out = fn(y)
        med_fb, _ = timeit(lambda: torch.autograd.grad(fn(y), y, g))
        med_b = med_fb - med_f
        line = f"maxavg B={B} N={N} C={C} {name:30s}: fwd {med_f:8.1f} us  bwd {med_b:8.1f} us (fwd+bwd {med_fb:8.1f})"
        if fwd_bytes:
            line += (f"  fwd {fwd_bytes / med_f / 1e3:6.0f} GB/s ({fwd_bytes / med_f / 8e6:.0%} of 8 TB/s)"
                     f"  bwd {bwd_bytes / med_b / 1e3:6.0f} GB/s ({bwd_bytes / med_b / 8e6:.0%})")
        print(line)
if "pmdist" in which:   # point-to-mesh distance: the kernel, a torch composition of the same math on the device, the fp64 CPU oracle
    import time
    import metrics_oracle as mo
    FLOP_PER_PAIR, PEAK = 110, 157.3e12   # nominal: ~65 VALU issues per pair evaluation, ~45 of them fma; fp32 vector peak of the guide
    torch.set_num_threads(16)

    def torch_form(p, v, f, chunk_pairs=8_000_000):   # the oracle's formula in fp32 on the device, chunked over queries
        tri = v[f.long()]
        step = max(1, chunk_pairs // len(tri))
        return torch.cat([mo.tri_dist2(p[i:i + step, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]).min(1).values
                          for i in range(0, len(p), step)]).sqrt()
    for name, B, P, s in (("pcae", 2, 2025, 45), ("grid64", 1, 20000, 64), ("odd", 3, 131, 3), ("eval", 1, 100000, 159)):
        verts, faces = mo.height_field_mesh(1, B, s)
        if name == "odd":
            faces = faces[:7]
        pts = mo.height_field_points(2, B, P) if name != "pcae" else verts + 0.01
        p, v, f = (torch.from_numpy(a).to(dev) for a in (pts.astype("float32"), verts, faces))
        Fn, pairs = len(faces), B * P * len(faces)
        med, mn = timeit(lambda: F.point_mesh_distance(p, v, f))
        med_all, _ = timeit(lambda: F.point_mesh_distance(p, v, f, return_face=True, return_closest=True))
        med_t, _ = timeit(lambda: [torch_form(p[b], v[b], f) for b in range(B)], iters=5, warm=1)
        nq = min(P, 500)   # the CPU oracle is timed on a slice of the queries of mesh 0 and scaled to all of them
        t0 = time.perf_counter()
        mo.point_mesh_dist2(pts[0][:nq], verts[0], faces)
        cpu_us = (time.perf_counter() - t0) * 1e6 * B * P / nq
        print(f"pmdist {name} B={B} P={P} F={Fn}: kernel median {med:9.1f} us (min {mn:9.1f}; with face+closest {med_all:9.1f})  "
              f"{pairs / med / 1e3:8.1f} G pair/s  {pairs * FLOP_PER_PAIR / (med * 1e-6) / PEAK:6.1%} of fp32 vector peak (nominal)  "
              f"torch composition {med_t:10.1f} us  fp64 CPU oracle, 16 threads ~{cpu_us:12.0f} us (scaled from {nq} queries)")
if "frontend" in which:
    # image front end (csrc/volume.hip) beside the torch composition of the same math on the same device (the oracle's fp32
    # code, tests/frontend_oracle.py): microseconds, GB/s against the compulsory bytes, peak device memory of both
    import json
    import frontend_oracle as fo
    from fissure_segmentation_amd.data_processing import foerstner, point_features
    shapes = [tuple(int(v) for v in a.split("x")) for a in os.environ.get("FSG_FRONTEND_SHAPES", "128x128x128,256x256x320,320x320x352").split(",")]

    def measure(fn, iters=10, warm=2):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        try:
            med, mn = timeit(fn, iters, warm)
        except torch.OutOfMemoryError:
            return None, None
        return med, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    def line(shape, name, bytes_needed, ours, theirs):
        rec = dict(kernel=name, shape="x".join(map(str, shape)), voxels=int(torch.tensor(shape).prod()))
        for tag, (us, mib) in (("hip", ours), ("torch", theirs)):
            rec[tag + "_us"] = None if us is None else round(us, 1)
            rec[tag + "_peak_MiB"] = None if mib is None else round(mib, 1)
            rec[tag + "_GBps"] = None if us is None else round(bytes_needed / us / 1e3, 1)
        print("FRONTEND " + json.dumps(rec), flush=True)

    for shape in shapes:
        img = fo.ct_volume(1, (32, 32, 32)).to(dev)
        img = torch.nn.functional.interpolate(img, size=shape, mode="trilinear") + 5 * torch.randn(1, 1, *shape, device=dev)
        mask = torch.ones(1, 1, *shape, dtype=torch.bool, device=dev)
        vox = img.numel()
        kp = torch.stack([torch.randint(0, s, (20000,), device=dev) for s in shape], 1)
        line(shape, "distinctiveness sigma=0.5", 8 * vox, measure(lambda: foerstner.distinctiveness(img, 0.5)),
             measure(lambda: fo.distinctiveness(img, 0.5)))
        line(shape, "foerstner_kpts sigma=0.5 d=5", 9 * vox, measure(lambda: foerstner.foerstner_kpts(img, mask, 0.5, 5)),
             measure(lambda: fo.foerstner_kpts(img, mask, 0.5, 5)))
        line(shape, "mind_at_keypoints K=20000", 4 * vox + 48 * 20000, measure(lambda: point_features.mind_at_keypoints(img, kp)),
             measure(lambda: fo.mind(img)[0][:, kp[:, 0], kp[:, 1], kp[:, 2]]))
        line(shape, "mind ssc", 52 * vox, measure(lambda: point_features.mind(img)), measure(lambda: fo.mind(img)))
if "hessian" in which:
    # Hessian fissure enhancement (csrc/fissure_enhance.hip) beside the torch composition of the same math on the same device
    # (the oracle's fp32 code, tests/hessian_oracle.py) over the whole volume -- None where its (D, H, W, 3, 3) tensor and the
    # eigvalsh workspace do not fit -- and beside the way the reference runs that composition on a GPU: over 64^3 patches with
    # an overlap of a quarter, blended with a Gaussian weight.
    import json
    import frontend_oracle as fo
    import hessian_oracle as ho
    from fissure_segmentation_amd.data_processing import keypoint_extraction as ke
    shapes = [tuple(int(v) for v in a.split("x")) for a in os.environ.get("FSG_FRONTEND_SHAPES", "128x128x128,256x256x320,320x320x352").split(",")]

    def measure(fn, iters=10, warm=2):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        try:
            med, mn = timeit(fn, iters, warm)
        except torch.OutOfMemoryError:
            return None, None
        return med, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    def patch_loop(img, patch=64, overlap=0.25):
        shape = img.shape[2:]
        out, weight = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        r = torch.arange(patch, device=dev) - (patch - 1) / 2
        g = torch.exp(-r ** 2 / (2 * (patch / 8) ** 2))
        g3 = g[:, None, None] * g[None, :, None] * g[None, None, :]
        starts = []
        for s in shape:
            n = max(1, -(-(s - patch) // int(patch * (1 - overlap))) + 1)
            starts.append(sorted({min(int(round(i * max(s - patch, 0) / max(n - 1, 1))), max(s - patch, 0)) for i in range(n)}))
        for z in starts[0]:
            for y in starts[1]:
                for x in starts[2]:
                    sl = (slice(z, z + patch), slice(y, y + patch), slice(x, x + patch))
                    p = ho.enhance(img[(slice(None), slice(None)) + sl])[0]
                    w = g3[: p.shape[0], : p.shape[1], : p.shape[2]]
                    out[sl] += p * w
                    weight[sl] += w
        return out / weight

    for shape in shapes:
        img = fo.ct_volume(1, (32, 32, 32)).to(dev)
        img = torch.nn.functional.interpolate(img, size=shape, mode="trilinear") + 5 * torch.randn(1, 1, *shape, device=dev)
        mask = torch.ones(1, 1, *shape, dtype=torch.bool, device=dev)
        vox = img.numel()
        enhanced = F.fissure_enhance(img, ho.MU, ho.SIGMA_HU, mask=mask)
        taps = F.discrete_gaussian_taps(1.0)
        rec = dict(kernel="fissure_enhance sigma=1", shape="x".join(map(str, shape)), voxels=vox)
        us, mib = measure(lambda: F.fissure_enhance(img, ho.MU, ho.SIGMA_HU))
        rec.update(hip_us=round(us, 1), hip_peak_MiB=round(mib, 1), hip_GBps=round(8 * vox / us / 1e3, 1))
        us, mib = measure(lambda: F.fissure_enhance(img, ho.MU, ho.SIGMA_HU, mask=mask, return_intermediate=True))
        rec.update(hip_masked_3out_us=round(us, 1), hip_masked_3out_peak_MiB=round(mib, 1))
        print("hessian: fused side of %s done, composition running" % rec["shape"], file=sys.stderr, flush=True)
        for tag, fn in (("torch", lambda: ho.enhance(img)[0]), ("torch_patch_loop", lambda: patch_loop(img))):
            us, mib = measure(fn, iters=3, warm=1)
            rec[tag + "_us"] = None if us is None else round(us, 1)
            rec[tag + "_peak_MiB"] = None if mib is None else round(mib, 1)
        print("HESSIAN " + json.dumps(rec), flush=True)
        rec = dict(kernel="smooth_threshold var=1 thresh=0.2", shape=rec["shape"], voxels=vox)
        us, mib = measure(lambda: F.smooth_threshold(enhanced, taps, 0.2))
        rec.update(hip_us=round(us, 1), hip_peak_MiB=round(mib, 1), hip_GBps=round(9 * vox / us / 1e3, 1))
        us, mib = measure(lambda: (ho.smooth(enhanced, taps) > 0.2))
        rec.update(torch_us=round(us, 1), torch_peak_MiB=round(mib, 1))
        print("HESSIAN " + json.dumps(rec), flush=True)
        values, flags = F.smooth_threshold(enhanced, taps, 0.2)
        ncand = int(flags.sum())
        rec = dict(kernel="hessian_enhancement_kpts K=20000", shape=rec["shape"], voxels=vox, candidates=ncand)
        us, mib = measure(lambda: ke.hessian_enhancement_kpts(enhanced))
        rec.update(hip_us=round(us, 1), hip_peak_MiB=round(mib, 1))
        cand = values.reshape(-1)[torch.nonzero(flags.reshape(-1)).squeeze(1)]
        us, _ = measure(lambda: torch.sort(cand, descending=True, stable=True))
        rec.update(candidate_sort_us=round(us, 1))
        us, mib = measure(lambda: torch.topk(ho.smooth(enhanced, taps).flatten(), 20000))
        rec.update(torch_dense_topk_us=round(us, 1), torch_peak_MiB=round(mib, 1))
        print("HESSIAN " + json.dumps(rec), flush=True)
if "cpd" in which:
    # CPD's E-step (csrc/cpd.hip) beside the torch composition of the same math on the same device (the oracle's fp32 formula,
    # batched: it materialises (B, M, N) tensors), with the peak extra device memory of both; then a whole 100-iteration
    # deformable registration at B = 32 and the share of it spent in the M x M solves (timed on their own, same matrices).
    import json
    import cpd_oracle as co
    from fissure_segmentation_amd.shape_model.point_cloud_registration import DeformableRegistration

    def measure(fn, iters=20, warm=3):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        med, _ = timeit(fn, iters, warm)
        return round(med, 1), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def torch_estep(X, TY, s2):
        K = torch.exp(-(X[:, None, :, :] - TY[:, :, None, :]).square().sum(3) / (2 * s2[:, None, None]))
        P = K / K.sum(1, keepdim=True)
        P1 = P.sum(2)
        return P1, P.sum(1), P @ X, P1.sum(1)

    def clouds(B, N, M):
        ps = [co.sheet_pair(N=N, M=M, seed=s) for s in range(B)]
        return torch.stack([p[0] for p in ps]).float().to(dev), torch.stack([p[1] for p in ps]).float().to(dev)

    for (B, N, M) in [(1, 1024, 1024), (32, 1024, 1024), (1, 3072, 3072)]:
        X, TY = clouds(B, N, M)
        s2 = torch.full((B,), 25., device=dev)
        rec = dict(kernel="cpd_estep sigma2=25 w=0", B=B, N=N, M=M, pairs=B * N * M)
        rec["hip_us"], rec["hip_peak_MiB"] = measure(lambda: F.cpd_estep(X, TY, s2))
        rec["torch_us"], rec["torch_peak_MiB"] = measure(lambda: torch_estep(X, TY, s2), iters=10, warm=2)
        # pair visits: the column launch sweeps every pair twice (minimum, then sum), the row launch once
        rec["hip_Gvisit_per_s"] = round(3 * B * N * M / rec["hip_us"] / 1e3, 1)
        print("CPD " + json.dumps(rec), flush=True)
    B, N, M, ITERATIONS, ALPHA = 32, 1024, 1024, 100, 0.01
    X, Y = clouds(B, N, M)
    reg = DeformableRegistration(X, Y, alpha=ALPHA, beta=10., max_iterations=ITERATIONS, tolerance=0)
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg.register()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    TY, (G, _) = reg.register()
    torch.cuda.synchronize()
    whole = time.perf_counter() - t1
    # one solve on its own, on the system of the last iteration: diag(P1) G + alpha sigma2 I, fp64
    sigma2 = reg.sigma2
    P1 = F.cpd_estep(X, TY, sigma2)[0].double()
    A = P1[:, :, None] * G.double() + (ALPHA * sigma2.double())[:, None, None] * torch.eye(M, dtype=torch.float64, device=dev)
    rhs = torch.randn(B, M, 3, dtype=torch.float64, device=dev)
    solve_us, _ = timeit(lambda: torch.linalg.solve_ex(A, rhs), iters=10, warm=2)
    print("CPD " + json.dumps(dict(kernel=f"deformable registration, {ITERATIONS} iterations", B=B, N=N, M=M,
                                   first_run_s=round(t1 - t0, 3), run_s=round(whole, 3), iterations=reg.iteration.tolist()[:4],
                                   solve_us_each=round(solve_us, 1),
                                   solves_fraction_of_run=round(ITERATIONS * solve_us * 1e-6 / whole, 3))), flush=True)
if "rw" in which:
    # random-walker lobe filling (csrc/random_walk.hip) beside the same Jacobi-preconditioned conjugate gradients written as a
    # torch composition on the same device (shifted-slice stencil over the whole volume, torch reductions, no host reads), run
    # for the iteration count the fused path needed.  Ellipsoid mask, K = 5 lobes, 2048 seeds, the binary graph of fill_lobes.
    import json, time, warnings
    import random_walk_oracle as ro
    shapes = [tuple(int(v) for v in a.split("x")) for a in os.environ.get("FSG_RW_SHAPES", "128x128x128,256x256x320").split(",")]
    K = 5

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(ts), out

    def peak(fn):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(); torch.cuda.synchronize()
        del out
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def torch_pcg(labels, mask, iters):
        im = labels != 0
        unknown, seeded = mask & ~im, mask & im
        w = [torch.where(im.narrow(a, 1, im.shape[a] - 1) == im.narrow(a, 0, im.shape[a] - 1), 1.0, 0.01) for a in range(3)]

        def nbr_sum(p):   # sum_j w_ij p_j over the axis neighbours, p (K, D, H, W)
            out = torch.zeros_like(p)
            for a in range(3):
                n = p.shape[a + 1] - 1
                out.narrow(a + 1, 1, n).add_(w[a] * p.narrow(a + 1, 0, n))
                out.narrow(a + 1, 0, n).add_(w[a] * p.narrow(a + 1, 1, n))
            return out
        diag = 1e-5 + nbr_sum(torch.ones(1, *im.shape, device=dev))[0]
        dinv = unknown / diag
        onehot = torch.stack([(seeded & (labels == k + 1)).float() for k in range(K)])
        r = nbr_sum(onehot) * unknown
        x, p = torch.zeros_like(r), dinv * r
        rz = (r * p).sum((1, 2, 3))
        for _ in range(iters):
            q = (diag * p - nbr_sum(p)) * unknown
            pq = (p * q).sum((1, 2, 3))
            alpha = torch.where(pq > 0, rz / pq, torch.zeros_like(pq))[:, None, None, None]
            x += alpha * p
            r -= alpha * q
            z = dinv * r
            rz2 = (r * z).sum((1, 2, 3))
            p = z + torch.where(rz > 0, rz2 / rz, torch.zeros_like(rz))[:, None, None, None] * p
            rz = rz2
        return x

    lines = []
    for shape in shapes:
        vol = ro.make_volume(shape, 2048, n_lobes=K, seed=0)
        labels, mask = torch.from_numpy(vol["labels"]).to(dev), torch.from_numpy(vol["mask"]).to(dev)
        V, U = labels.numel(), int((mask & (labels == 0)).sum())
        solve = lambda **kw: F.random_walk_fill(labels, mask, num_labels=K, return_info=True, **kw)
        solve(); solve()   # warm-up
        us, (filled, info) = wall(solve)
        iters = info["iterations"].tolist()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # tol = 0 never stops: every system stays live, the count is fixed
            n_it = 100
            us0, _ = wall(lambda: solve(tol=0.0, max_iter=0))
            us1, _ = wall(lambda: solve(tol=0.0, max_iter=n_it, check_every=n_it))
        us_iter = (us1 - us0) / n_it
        bytes_iter = U * (40 * K + 9) + 2 * V   # vectors of the unknown voxels, their image byte and inverse diagonal, every state byte twice
        rec = dict(kernel="random_walk_fill binary K=5 seeds=2048 tol=1e-3", shape="x".join(map(str, shape)), voxels=V, unknowns=U,
                   iterations=iters, relative_residual=[round(v, 6) for v in info["relative_residual"].tolist()],
                   hip_solve_us=round(us, 1), hip_setup_and_finish_us=round(us0, 1), hip_us_per_iteration_all_live=round(us_iter, 1),
                   bytes_per_iteration=bytes_iter, hip_GBps=round(bytes_iter / us_iter / 1e3, 1),
                   hip_share_of_6p29TBps=round(bytes_iter / us_iter / 6.29e6, 3),
                   hip_workspace_MiB=round(fsg._lib.lib.fsg_random_walk_workspace_bytes(1, K, *shape) / 2 ** 20, 1))
        rec["hip_peak_MiB"] = peak(solve)
        print("rw: fused side of %s done, composition running" % rec["shape"], file=sys.stderr, flush=True)
        n = max(iters)
        torch_pcg(labels, mask, 2)   # warm-up
        tus, _ = wall(lambda: torch_pcg(labels, mask, n), reps=3)
        tus0, _ = wall(lambda: torch_pcg(labels, mask, 0), reps=3)
        rec.update(torch_iterations=n, torch_solve_us=round(tus, 1), torch_us_per_iteration=round((tus - tus0) / n, 1),
                   torch_peak_MiB=peak(lambda: torch_pcg(labels, mask, 2)))
        rec["speedup_same_iterations"] = round(tus / us, 2)
        print("RW " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    out_path = os.environ.get("FSG_RW_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "morph" in which:
    # ball morphology and connected components on bit planes (csrc/morphology.hip) beside (a) the torch composition on the same
    # device -- conv3d of the fp16 volume with the ball as kernel, thresholded, as the reference's own dilation in
    # lobes_to_fissures does; there is no torch composition of connected components, so that stage has the host baseline only --
    # and (b) scipy.ndimage on the host.  Input: the synthetic two-lung volume of the tests scaled to the shape.
    import json, time
    import numpy as np
    import morphology_oracle as mo
    from fissure_segmentation_amd.data_processing import find_lobes as fl
    shapes = [tuple(int(v) for v in a.split("x")) for a in os.environ.get("FSG_MORPH_SHAPES", "128x128x128,256x256x320").split(",")]
    with_host = os.environ.get("FSG_MORPH_HOST", "1") != "0"

    def wall(fn, reps=5):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(ts), out

    def peak(fn):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(); torch.cuda.synchronize()
        del out
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def host(fn):
        t0 = time.perf_counter(); out = fn()
        return (time.perf_counter() - t0) * 1e6, out

    def t_dilate(x, r, border=0):   # x (1, 1, D, H, W) fp16 0 / 1
        k = torch.from_numpy(mo.ball(r)).to(dev, torch.float16)[None, None]
        xp = torch.nn.functional.pad(x, (r,) * 6, value=float(border))
        return (torch.nn.functional.conv3d(xp, k) > 0).to(torch.float16)

    def t_erode(x, r, border=1):
        return 1 - t_dilate(1 - x, r, 1 - border)

    def t_closing(x, r):
        p = torch.nn.functional.pad(x, (r,) * 6)
        return t_erode(t_dilate(p, r), r, 0)[..., r:-r, r:-r, r:-r]

    def t_opening(x, r):
        return t_dilate(t_erode(x, r, 0), r)

    lines = []
    for shape in shapes:
        lung, fis = mo.lung_volume(shape)
        tl, tf = torch.from_numpy(lung).to(dev), torch.from_numpy(fis).to(dev)
        W = shape[-1]
        not_lobes_np = ~mo.erode(lung, 2, 1) | (fis != 0) if with_host else None
        bits = F._pack_bits(tl[None])
        nl_bits = F._bits_dilate(bits, W, (2, 2, 2), border=0, inv_in=True) | F._pack_bits(tf[None])
        nl16 = F._unpack_bits(nl_bits, W)[None].to(torch.float16)
        lm_bits = F._bits_dilate(F._bits_closing(nl_bits, W, (2, 2, 2)), W, (2, 2, 2), border=0, inv_out=True)
        lm16 = F._unpack_bits(lm_bits, W)[None].to(torch.float16)
        open_bits = F._bits_opening(lm_bits, W, (4, 4, 4))
        rec = dict(kernel="ball morphology + connected components on bit planes", shape="x".join(map(str, shape)),
                   voxels=int(np.prod(shape)))
        stages = {
            "closing_r2": (lambda: F._bits_closing(nl_bits, W, (2, 2, 2)), lambda: t_closing(nl16, 2)),
            "opening_r4": (lambda: F._bits_opening(lm_bits, W, (4, 4, 4)), lambda: t_opening(lm16, 4)),
            "components": (lambda: F._cc_bits(open_bits, W, 6), None),
            "find_lobes": (lambda: fl.find_lobes(tf, tl), None),
        }
        for name, (fused, comp) in stages.items():
            fused(); fused()
            us, out = wall(fused)
            rec[f"{name}_hip_us"] = round(us, 1)
            rec[f"{name}_hip_peak_MiB"] = peak(fused)
            if comp is not None:
                comp(); ref = comp()
                same = torch.equal(F._unpack_bits(out, W)[None], ref > 0)
                tus, _ = wall(comp, reps=3)
                rec[f"{name}_torch_us"] = round(tus, 1)
                rec[f"{name}_torch_peak_MiB"] = peak(comp)
                rec[f"{name}_speedup_vs_torch"] = round(tus / us, 2)
                rec[f"{name}_equals_torch"] = bool(same)
            print("morph: %s %s done" % (rec["shape"], name), file=sys.stderr, flush=True)
        rec["find_lobes_components"] = int(F._cc_bits(open_bits, W, 6)[1][0])
        # find_lobes as a torch composition: its four morphology steps (the component stage has none)
        def t_chain():
            nl = t_dilate(t_closing(torch.maximum(1 - t_erode(tl[None, None].to(torch.float16), 2, 1),
                                                   (tf != 0)[None, None].to(torch.float16)), 2), 2)
            return t_opening(1 - nl, 4)
        t_chain()
        tus, ref = wall(t_chain, reps=3)
        rec["find_lobes_morphology_torch_us"] = round(tus, 1)
        rec["find_lobes_morphology_torch_peak_MiB"] = peak(t_chain)
        rec["find_lobes_morphology_equals_torch"] = bool(torch.equal(F._unpack_bits(open_bits, W)[None], ref > 0))
        if with_host:
            hus, c_np = host(lambda: mo.closing(not_lobes_np, 2)); rec["closing_r2_scipy_us"] = round(hus, 1)
            lm_np = ~mo.dilate(c_np, 2, 0)
            hus, o_np = host(lambda: mo.opening(lm_np, 4)); rec["opening_r4_scipy_us"] = round(hus, 1)
            hus, (lab_np, n_np) = host(lambda: mo.label(o_np, 6)); rec["components_scipy_us"] = round(hus, 1)
            hus, (lobes_np, ok) = host(lambda: mo.find_lobes(fis, lung)); rec["find_lobes_scipy_us"] = round(hus, 1)
            got, _, ok_hip = fl.find_lobes(tf, tl)
            rec["find_lobes_equals_scipy"] = bool(ok == ok_hip and np.array_equal(got.cpu().numpy(), lobes_np))
            rec["components_equal_scipy"] = bool(np.array_equal(F._cc_bits(open_bits, W, 6)[0][0].cpu().numpy(), lab_np))
        print("MORPH " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    out_path = os.environ.get("FSG_MORPH_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "edt" in which:
    # Euclidean distance transform (csrc/edt.hip), nearest_label and the lung split on top of it, beside
    # scipy.ndimage.distance_transform_edt on the host in the same run (there is no torch composition of an exact EDT).
    # Masks: (a) the synthetic two-lung volume of the tests scaled to the shape (sites = everything outside the lungs),
    # (b) the worst case of the outward walk, one site in a corner of a set volume.  FSG_EDT_HOST=0 leaves the host runs out.
    import json, time
    import numpy as np
    from scipy import ndimage as ndi
    import edt_oracle as eo
    import morphology_oracle as mo
    from fissure_segmentation_amd.data_processing import process_lung_mask as plm
    shapes = [tuple(int(v) for v in a.split("x")) for a in os.environ.get("FSG_EDT_SHAPES", "128x128x128,256x256x320").split(",")]
    with_host = os.environ.get("FSG_EDT_HOST", "1") != "0"
    spacing = (2.5, 1.0, 0.75)

    def peak(fn):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(); torch.cuda.synchronize()
        del out
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def host(fn):
        t0 = time.perf_counter(); out = fn()
        return round((time.perf_counter() - t0) * 1e6, 1), out

    lines = []
    for shape in shapes:
        D, H, W = shape
        V = D * H * W
        lung = mo.lung_volume(shape)[0]
        corner = np.ones(shape, bool)
        corner[0, 0, 0] = False
        bridged = lung.copy()
        bridged[D // 2 - 1:D // 2 + 2, H // 2 - 1:H // 2 + 2, int(W * 0.26):int(W * 0.74)] = True     # a bar three voxels thick
        rec = dict(kernel="Euclidean distance transform on bit planes", shape="x".join(map(str, shape)), voxels=V,
                   compulsory_MB=round((V / 8 + 4 * V + 2 * 8 * V) / 1e6, 1), compulsory_with_indices_MB=round(
                       (V / 8 + 4 * V + 12 * V + 2 * 16 * V) / 1e6, 1))
        for mname, m in (("lungs", lung), ("corner", corner)):
            t = torch.from_numpy(m).to(dev)
            bits = F._pack_bits(t[None])
            for vname, s, want_idx in (("unit", None, False), ("unit_idx", None, True), ("spacing", spacing, False),
                                       ("spacing_idx", spacing, True)):
                key = f"{mname}_{vname}"
                med, mn = timeit(lambda: F._edt_bits(bits, W, s, want_idx), iters=10, warm=2)
                rec[f"{key}_kernels_us"] = round(med, 1)
                med, mn = timeit(lambda: F.distance_transform_edt(t, sampling=s, return_indices=want_idx), iters=10, warm=2)
                rec[f"{key}_hip_us"] = round(med, 1)
                rec[f"{key}_hip_peak_MiB"] = peak(lambda: F.distance_transform_edt(t, sampling=s, return_indices=want_idx))
                print("edt: %s %s done" % (rec["shape"], key), file=sys.stderr, flush=True)
            rec[f"{mname}_unit_kernels_GBps_of_compulsory"] = round(rec["compulsory_MB"] * 1e6 / (rec[f"{mname}_unit_kernels_us"] * 1e-6) / 1e9, 1)
            if with_host:
                hus, ref = host(lambda: ndi.distance_transform_edt(m))
                rec[f"{mname}_unit_scipy_us"] = hus
                rec[f"{mname}_unit_speedup_vs_scipy"] = round(hus / rec[f"{mname}_unit_hip_us"], 1)
                got = F.distance_transform_edt(t, squared=True).cpu().numpy()
                rec[f"{mname}_unit_equals_scipy"] = bool(np.array_equal(got, np.rint(ref ** 2).astype(np.int32)))
                if mname == "lungs":
                    hus, ref = host(lambda: ndi.distance_transform_edt(m, sampling=spacing, return_indices=True))
                    rec["lungs_spacing_idx_scipy_us"] = hus
                    rec["lungs_spacing_idx_speedup_vs_scipy"] = round(hus / rec["lungs_spacing_idx_hip_us"], 1)
                    got = F.distance_transform_edt(t, sampling=spacing, squared=True).cpu().numpy().astype(np.float64)
                    rec["lungs_spacing_max_rel_err"] = float(np.max(np.abs(got - ref[0] ** 2)[ref[0] > 0] / ref[0][ref[0] > 0] ** 2))
                del ref, got
        # nearest_label with two labels: the restoration step of the lung split (sites = the voxels of each lung)
        lab = torch.from_numpy(mo.label(lung, 6)[0]).to(dev)
        med, mn = timeit(lambda: F.nearest_label(lab, (1, 2)), iters=10, warm=2)
        rec["nearest_label2_hip_us"] = round(med, 1)
        rec["nearest_label2_hip_peak_MiB"] = peak(lambda: F.nearest_label(lab, (1, 2)))
        tb = torch.from_numpy(bridged).to(dev)
        import contextlib, io
        def split():
            with contextlib.redirect_stdout(io.StringIO()):
                return plm.binary_lung_mask_to_left_right(tb)
        out = split()
        rec["lung_split_opened"] = bool(F.connected_components(tb)[1] == 1)
        med, mn = timeit(split, iters=5, warm=1)
        rec["lung_split_hip_us"] = round(med, 1)
        rec["lung_split_hip_peak_MiB"] = peak(split)
        if with_host:
            lab_np = lab.cpu().numpy()
            hus, ref = host(lambda: eo.nearest_label(lab_np, (1, 2)))
            rec["nearest_label2_scipy_us"] = hus
            rec["nearest_label2_speedup_vs_scipy"] = round(hus / rec["nearest_label2_hip_us"], 1)
            rec["nearest_label2_equals_scipy"] = bool(np.array_equal(F.nearest_label(lab, (1, 2)).cpu().numpy(), ref))
            hus, (ref, radii, _) = host(lambda: eo.lung_split(bridged))
            rec["lung_split_scipy_us"] = hus
            rec["lung_split_speedup_vs_scipy"] = round(hus / rec["lung_split_hip_us"], 1)
            rec["lung_split_equals_scipy"] = bool(np.array_equal(out.cpu().numpy(), ref))
            rec["lung_split_scipy_radii"] = radii
        print("EDT " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    out_path = os.environ.get("FSG_EDT_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "thin" in which:
    # In-plane binary thinning (csrc/thinning.hip): whole `binary_thinning` calls and the thinning launch alone, beside (a) the
    # torch composition of the same rule on the device (replicate-padded shifted slices, one host read per pair) and (b) the numpy
    # oracle on the host (tests/thinning_oracle.py; it stands in for ITK, which is not available), in the same run.  Inputs: a
    # synthetic three-sheet fissure label map, 3-5 voxels thick, as three planes in one launch, and the synthetic two-lung mask
    # as the deep case.  Then the stage split of a whole poisson_reconstruction.  FSG_THIN_HOST=0 leaves the host runs out.
    import json, time
    import numpy as np
    import morphology_oracle as mo
    import thinning_oracle as tho
    from fissure_segmentation_amd.data_processing.poisson_reconstruction import poisson_reconstruction
    shapes = [tuple(int(v) for v in a.split("x")) for a in os.environ.get("FSG_THIN_SHAPES", "128x128x128,256x256x320").split(",")]
    with_host = os.environ.get("FSG_THIN_HOST", "1") != "0"
    host_max = int(os.environ.get("FSG_THIN_HOST_MAX_VOXELS", 128 ** 3))   # numpy needs seconds per step on 2 10^7 voxels

    def peak(fn):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(); torch.cuda.synchronize()
        del out
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def three_sheets(shape):
        D, H, W = shape
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij", sparse=True)
        lab = np.zeros(shape, np.int64)
        lab[(np.abs(y - (0.35 * H + 0.2 * x + 0.1 * z + 2 * np.sin(x / 9.0))) <= 1.5) & (x < W // 2 - 4) & (x > 4)] = 1
        lab[(np.abs(y - (0.30 * H + 0.25 * (x - W / 2) + 0.1 * z)) <= 2.0) & (x > W // 2 + 4) & (x < W - 4)] = 2
        lab[(np.abs(y - (0.75 * H - 0.2 * (x - W / 2) - 0.05 * z)) <= 2.5) & (x > W // 2 + 4) & (x < W - 4)] = 3
        return lab

    def torch_thin(v):
        """the rule composed from torch operations: v (S, H, W) bool -> (thinned, pairs per slice); one host read per pair"""
        pad = torch.nn.functional.pad
        img = v.to(torch.uint8)
        pairs = torch.zeros(img.shape[0], dtype=torch.int32, device=img.device)
        H, W = img.shape[-2:]
        for _ in range(H * W + 1):
            cleared = torch.zeros(img.shape[0], dtype=torch.bool, device=img.device)
            for odd in (True, False):
                p = pad(img[:, None].float(), (1, 1, 1, 1), mode="replicate")[:, 0].to(torch.uint8)
                n8 = [p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in tho.OFFSETS]
                p2, p3, p4, p5, p6, p7, p8, p9 = n8
                cnt = sum(q.to(torch.int32) for q in n8)
                trans = sum(((n8[k] == 0) & (n8[(k + 1) % 8] == 1)).to(torch.int32) for k in range(8))
                cd = ((p2 & p4 & p6) == 0) & ((p4 & p6 & p8) == 0) if odd else ((p2 & p4 & p8) == 0) & ((p2 & p6 & p8) == 0)
                mark = (img == 1) & (cnt >= 2) & (cnt <= 6) & (trans == 1) & cd
                cleared |= mark.flatten(1).any(1)
                img = img & ~mark.to(torch.uint8)
            if not bool(cleared.any()):                              # the host read
                break
            pairs += cleared
        return img.bool(), pairs

    lines = []
    for shape in shapes:
        D, H, W = shape
        lab = three_sheets(shape)
        lung = mo.lung_volume(shape)[0]
        rec = dict(kernel="in-plane binary thinning on bit planes", shape="x".join(map(str, shape)), voxels=D * H * W)
        cases = (("sheets3", torch.from_numpy(np.stack([lab == f for f in (1, 2, 3)])).to(dev)),
                 ("lungs", torch.from_numpy(lung).to(dev)[None]))
        for cname, t in cases:
            bits = F._pack_bits(t)
            out, it = F.binary_thinning(t, return_iterations=True)
            rec[f"{cname}_pairs_max"], rec[f"{cname}_pairs_mean"] = int(it.max()), round(float(it.float().mean()), 2)
            rec[f"{cname}_voxels_in"], rec[f"{cname}_voxels_out"] = int(t.sum()), int(out.sum())
            rec[f"{cname}_compulsory_MB"] = round(2 * t.numel() / 1e6, 1)       # a byte in and a byte out around the 1-bit plane
            med, mn = timeit(lambda: F._bits_thin(bits, W), iters=20, warm=3)
            rec[f"{cname}_launch_us"] = round(med, 1)
            med, mn = timeit(lambda: F.binary_thinning(t), iters=20, warm=3)
            rec[f"{cname}_hip_us"] = round(med, 1)
            rec[f"{cname}_hip_peak_MiB"] = peak(lambda: F.binary_thinning(t))
            flat = t.reshape(-1, H, W)
            ref, rp = torch_thin(flat)
            rec[f"{cname}_equals_torch"] = bool(torch.equal(ref.reshape(t.shape), out) and torch.equal(rp.reshape(it.shape), it))
            med, mn = timeit(lambda: torch_thin(flat), iters=3, warm=1)
            rec[f"{cname}_torch_us"] = round(med, 1)
            rec[f"{cname}_torch_peak_MiB"] = peak(lambda: torch_thin(flat))
            rec[f"{cname}_speedup_vs_torch"] = round(rec[f"{cname}_torch_us"] / rec[f"{cname}_hip_us"], 1)
            del ref, rp
            print("thin: %s %s done" % (rec["shape"], cname), file=sys.stderr, flush=True)
            if with_host and D * H * W <= host_max:
                m = t.cpu().numpy()
                t0 = time.perf_counter(); want, wp = tho.thin(m)
                rec[f"{cname}_numpy_us"] = round((time.perf_counter() - t0) * 1e6, 1)
                rec[f"{cname}_speedup_vs_numpy"] = round(rec[f"{cname}_numpy_us"] / rec[f"{cname}_hip_us"], 1)
                rec[f"{cname}_equals_numpy"] = bool(np.array_equal(out.cpu().numpy(), want) and np.array_equal(it.cpu().numpy(), wp))
                del want, wp
        if shape == shapes[-1]:
            labels = torch.from_numpy(lab).to(dev)
            mask = torch.ones(shape, dtype=torch.bool, device=dev)
            poisson_reconstruction(labels, mask, (1.0, 1.0, 1.0))                                    # warm-up
            _, meshes, times = poisson_reconstruction(labels, mask, (1.0, 1.0, 1.0), return_times=True)
            rec["poisson_reconstruction_stage_s"] = {k: round(v, 4) for k, v in times.items()}
            rec["poisson_reconstruction_faces"] = meshes.num_faces_per_mesh().tolist()
        print("THIN " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    out_path = os.environ.get("FSG_THIN_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "mesh" in which:
    # mesh regularisers, surface sampler and the whole default mesh loss (csrc/mesh.hip) beside the torch composition of the
    # same math on the same device (the oracle's fp32 code, tests/mesh_oracle.py, batched over the shared face list), value +
    # gradient, with the peak extra device memory of both.  B = 32 is the training step of train_pc_ae.py --loss mesh.
    import json
    import mesh_oracle as mo
    from fissure_segmentation_amd.losses.mesh_loss import RegularizedMeshLossHIP
    from fissure_segmentation_amd.mesh import Meshes, mesh_regularizers, sample_points_from_uniforms
    from fissure_segmentation_amd.shapes.shape_constructor import get_plane_mesh

    def measure(fn, iters=50, warm=5):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        med, _ = timeit(fn, iters, warm)
        return round(med, 1), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)

    lines = []
    n_samples = 2048
    for B in (32, 1):
        p, faces = get_plane_mesh(2048, xrange=(-0.3, 0.3), yrange=(-0.3, 0.3))
        faces = faces.to(dev)
        verts = torch.cat([p, torch.zeros(len(p), 1)], 1).to(dev)[None].repeat(B, 1, 1)
        verts = (verts + 0.01 * torch.randn(B, len(p), 3, device=dev)).requires_grad_(True)
        target = (verts.detach() * 0.9 + 0.02).contiguous()
        topo = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in mo.brute_topology(faces, len(p)).items()}
        u = torch.rand(B, n_samples, 3, device=dev)
        g = torch.randn(B, n_samples, 3, device=dev)
        fl = faces.long()

        def t_terms(v):        # mesh_oracle.mesh_terms, batched: (B, V, 3) -> three batch means
            e, pr = topo["edges"], topo["pairs"]
            edge = (v[:, e[:, 0]] - v[:, e[:, 1]]).square().sum(2).mean(1).mean()
            v0, ed = v[:, pr[:, 0]], v[:, pr[:, 1]] - v[:, pr[:, 0]]
            n0, n1 = torch.linalg.cross(ed, v[:, pr[:, 2]] - v0), -torch.linalg.cross(ed, v[:, pr[:, 3]] - v0)
            normal = (1 - torch.nn.functional.cosine_similarity(n0, n1, dim=2)).mean(1).mean()
            s = torch.zeros_like(v).index_add(1, topo["src"], v[:, topo["dst"]])
            lap = (s / topo["deg"].clamp(min=1)[None, :, None] - v).norm(dim=2).mean(1).mean()
            return edge, normal, lap

        def t_sample(v, u):    # mesh_oracle.sample, batched
            tri = v[:, fl]
            area = 0.5 * torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]).double().norm(dim=2)
            C = torch.cumsum(area.detach(), 1)
            face = torch.searchsorted(C, u[:, :, 0].double() * C[:, -1:], right=True).clamp(max=fl.shape[0] - 1)
            r = u[:, :, 1].sqrt()
            w = torch.stack([1 - r, r * (1 - u[:, :, 2]), r * u[:, :, 2]], 2)
            corners = torch.gather(v[:, fl].flatten(2), 1, face[:, :, None].expand(-1, -1, 9)).unflatten(2, (3, 3))
            return (corners * w[:, :, :, None]).sum(2)

        def t_chamfer(x, y):
            d = torch.cdist(x, y).square()
            return d.min(2).values.mean(1).mean() + d.min(1).values.mean(1).mean()

        def hip_reg():
            e, n, l = mesh_regularizers(Meshes(verts, faces))
            return torch.autograd.grad(e + 0.1 * n + 0.1 * l, verts)

        def torch_reg():
            e, n, l = t_terms(verts)
            return torch.autograd.grad(e + 0.1 * n + 0.1 * l, verts)

        def hip_sample():
            return torch.autograd.grad(sample_points_from_uniforms(Meshes(verts, faces), u), verts, g)

        def torch_sample():
            return torch.autograd.grad(t_sample(verts, u), verts, g)

        loss_fn = RegularizedMeshLossHIP()

        def hip_loss():
            return torch.autograd.grad(loss_fn(Meshes(verts, faces), Meshes(target, faces))[0], verts)

        def torch_loss():
            e, n, l = t_terms(verts)
            u1, u2 = torch.rand(B, n_samples, 3, device=dev), torch.rand(B, n_samples, 3, device=dev)
            c = t_chamfer(t_sample(verts, u1), t_sample(target, u2))
            return torch.autograd.grad(c + e + 0.1 * n + 0.1 * l, verts)

        for stage, ours, theirs in (("regularisers value+grad", hip_reg, torch_reg), ("sampler fwd+bwd", hip_sample, torch_sample),
                                    ("default loss fwd+bwd", hip_loss, torch_loss)):
            rec = dict(kernel="mesh " + stage, B=B, V=len(p), F=int(faces.shape[0]), n_samples=n_samples)
            rec["hip_us"], rec["hip_peak_MiB"] = measure(ours)
            rec["torch_us"], rec["torch_peak_MiB"] = measure(theirs)
            rec["speedup"] = round(rec["torch_us"] / rec["hip_us"], 2)
            print("MESH " + json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        fsg._lib.start_timing()
        for _ in range(20):
            hip_loss()
        for name, v in fsg._lib.stop_timing().items():
            rec = dict(kernel="mesh default loss: " + name, B=B, calls_per_step=len(v) // 20,
                       median_us=round(1e3 * sorted(v)[len(v) // 2], 1))
            print("MESH " + json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    out_path = os.environ.get("FSG_MESH_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "dpsr" in which:
    # the DPSR front (csrc/grid_points.hip) beside the torch composition of the same math on the same device, fp32, with the peak
    # extra device memory of both: 'torch' mode against F.grid_sample and its autograd adjoint, 'sap' mode against the
    # reference-style scatter_add_ / gather (tests/dpsr_oracle.py), the spectral solve against the complex composition, and
    # DPSR.forward / SoftMesh.psr_grid with their backward against the oracle's whole composition.  8 x 2048 points at 128^3,
    # sigma 10, C in {3, 5}, one item alone, and a cloud whose points all share one cell.  The one-axis Gaussian derivative and
    # the FFT stay torch's in both columns: their share of SoftMesh.psr_grid is reported on its own lines.
    import json
    import torch.nn.functional as TF
    import dpsr_oracle as do
    from fissure_segmentation_amd.models.dpsr_net import DPSR
    from fissure_segmentation_amd.models.seg_logits_to_mesh import SoftMesh
    from fissure_segmentation_amd.utils.image_utils import gaussian_differentiation

    def measure(fn, iters=20, warm=3):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        med, _ = timeit(fn, iters, warm)
        return round(med, 1), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)

    lines = []

    def report(stage, ours, theirs, iters=20, **shape):
        rec = dict(kernel="dpsr " + stage, **shape)
        rec["hip_us"], rec["hip_peak_MiB"] = measure(ours, iters)
        rec["torch_us"], rec["torch_peak_MiB"] = measure(theirs, iters)
        rec["speedup"] = round(rec["torch_us"] / rec["hip_us"], 2)
        print("DPSR " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    res, sig, N = (128, 128, 128), 10, 2048
    gen = torch.Generator().manual_seed(0)
    for B, C, cloud_kind in [(8, 3, "uniform"), (8, 5, "uniform"), (1, 3, "uniform"), (1, 5, "uniform"), (8, 5, "one cell")]:
        for mode in ("torch", "sap"):
            if cloud_kind == "uniform":
                lo, hi = (-1.0, 1.0) if mode == "torch" else (0.0, 1.0)
                x = (torch.rand(B, N, 3, generator=gen) * (hi - lo) + lo).to(dev)
            else:
                x = do.one_cell_coords(mode).expand(B, -1, -1).contiguous().to(dev)
            v = torch.randn(B, C, N, generator=gen).to(dev)
            grid = torch.randn(B, C, *res, device=dev)
            g = torch.randn(B, C, N, device=dev)
            x5 = x.view(B, N, 1, 1, 3)
            shape = dict(mode=mode, B=B, C=C, N=N, res=128, cloud=cloud_kind)

            def torch_splat():
                if mode == "sap":
                    return do.splat(v, x, res, "sap")
                z = torch.zeros(B, C, *res, device=dev, requires_grad=True)
                return torch.autograd.grad(TF.grid_sample(z, x5, align_corners=False), z, v.view(B, C, N, 1, 1))[0]
            report("splat", lambda: F.splat_to_grid(v, x, res, mode), torch_splat, **shape)
            if cloud_kind == "one cell":
                continue
            xr = x.clone().requires_grad_(True)

            def hip_sample():
                s = F.sample_grid(grid, xr, mode)
                return s, torch.autograd.grad(s, xr, g)

            def torch_sample():
                s = do.sample(grid, xr, "sap") if mode == "sap" else \
                    TF.grid_sample(grid, xr.view(B, N, 1, 1, 3), align_corners=False).view(B, C, N)
                return s, torch.autograd.grad(s, xr, g)
            report("sample + coordinate gradient", hip_sample, torch_sample, **shape)
    for B in (8, 1):
        nhat = torch.fft.rfftn(torch.randn(B, 3, *res, device=dev), dim=(2, 3, 4))
        report("spectral solve", lambda: F.psr_spectral_solve(nhat, res, sig), lambda: do.spectral(nhat, res, sig), B=B, res=128,
               sig=sig)
        s = do.sphere_case(B=B, N=N)
        V, Nn = s["V"].to(dev).requires_grad_(True), s["N"].to(dev).requires_grad_(True)
        gphi = torch.randn(B, *res, device=dev)
        net = DPSR(res, sig).to(dev)
        report("DPSR.forward + backward", lambda: torch.autograd.grad(net(V, Nn), (V, Nn), gphi),
               lambda: torch.autograd.grad(do.dpsr(V, Nn, res, sig), (V, Nn), gphi), iters=10, B=B, N=N, res=128, sig=sig)
        fsg._lib.start_timing()
        for _ in range(10):
            torch.autograd.grad(net(V, Nn), (V, Nn), gphi)
        for name, t in fsg._lib.stop_timing().items():
            rec = dict(kernel="dpsr DPSR.forward + backward: " + name, B=B, calls_per_step=len(t) // 10,
                       median_us=round(1e3 * sorted(t)[len(t) // 2], 1))
            print("DPSR " + json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    for B, C in [(8, 3), (1, 3), (1, 5)]:
        m = do.softmesh_case(B=B, K=C + 1, N=N)
        lg, xc = m["logits"].to(dev).requires_grad_(True), m["coords"].to(dev)
        gf = torch.randn(B * C, *res, device=dev)
        sm = SoftMesh(10, res, sig).to(dev)
        report("SoftMesh.psr_grid + backward", lambda: torch.autograd.grad(sm.psr_grid(lg, xc), lg, gf),
               lambda: torch.autograd.grad(do.softmesh_field(lg, xc, res, 10, sig), lg, gf), iters=5, B=B, C=C, N=N, res=128, sig=sig)
        seg = torch.randn(B, C, *res, device=dev, requires_grad=True)
        gn = torch.randn(B, C, 3, *res, device=dev)

        def conv_part():
            n = torch.stack([gaussian_differentiation(seg, 10, 1, d, 'constant', 1.5) for d in (2, 1, 0)], 2)
            return torch.autograd.grad(n, seg, gn)
        fld = torch.randn(B * C, 3, *res, device=dev, requires_grad=True)
        gh = torch.randn(B * C, *res, device=dev)

        def fft_part():
            h = torch.fft.rfftn(fld, dim=(2, 3, 4))
            return torch.autograd.grad(torch.fft.irfftn(h[:, 0] + h[:, 1] + h[:, 2], s=res, dim=(1, 2, 3)), fld, gh)
        for part, fn in (("Gaussian derivative (torch conv3d) fwd+bwd", conv_part), ("rfftn + irfftn fwd+bwd", fft_part)):
            us, peak = measure(fn, 5)
            rec = dict(kernel="dpsr SoftMesh.psr_grid share: " + part, B=B, C=C, res=128, torch_us=us, torch_peak_MiB=peak)
            print("DPSR " + json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    out_path = os.environ.get("FSG_DPSR_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "mc" in which:
    # marching cubes (csrc/marching_cubes.hip): HIP-event medians of the whole call (its one host read included) and of its two
    # C-ABI halves, vertex and face counts, bytes moved against the compulsory bytes (the field once, the outputs once), peak
    # extra device memory, the numpy oracle on the CPU for scale, and SoftMesh.meshes beside SoftMesh.psr_grid (forward +
    # backward) from the same run.  No device composition of marching cubes exists to race (pytorch3d and scikit-image are not
    # installed), so there is no second column.
    import json
    import time
    import numpy as np
    import dpsr_oracle as do
    import mc_oracle as mo
    from fissure_segmentation_amd.models.seg_logits_to_mesh import SoftMesh

    def measure(fn, iters=10, warm=2):
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        med, _ = timeit(fn, iters, warm)
        return round(med, 1), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)

    lines = []

    def emit_line(rec):
        print("MC " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    def stage_times(fn, reps=5):
        fsg._lib.start_timing()
        for _ in range(reps):
            fn()
        return {k: round(1e3 * sorted(v)[len(v) // 2], 1) for k, v in fsg._lib.stop_timing().items() if k.startswith("fsg_mc_")}

    res, sig, N = (128, 128, 128), 10, 2048
    fields = {}
    for B, C in [(1, 1), (8, 3)]:
        m = do.softmesh_case(B=B, K=C + 1, N=N)
        sm = SoftMesh(10, res, sig).to(dev)
        with torch.no_grad():
            fields[B * C] = sm.psr_grid(m["logits"].to(dev), m["coords"].to(dev)).contiguous()
    for n_fields, field in fields.items():
        v, f, n, nv, nf = F.marching_cubes(field)
        nodes = field.numel()
        out_bytes = v.numel() * 4 * 2 + f.numel() * 8
        # count: field 8 corner reads (once from HBM, the rest cache hits) + 1 B case + 7 B cases + 2 B code per node; emit: 2 B code
        # twice + 1 B case twice per node, the field at the crossing edges, the outputs once, the vertices again for the normals
        moved = nodes * (4 + 1 + 1 + 2 + 2 + 2 + 1 + 1) + out_bytes + sum(nf) * 3 * 12
        us, peak = measure(lambda: F.marching_cubes(field))
        rec = dict(kernel="mc marching_cubes (count + host read + emit)", fields=n_fields, res=128, hip_us=us, hip_peak_MiB=peak,
                   verts=sum(nv), faces=sum(nf), compulsory_MB=round((nodes * 4 + out_bytes) / 1e6, 2),
                   moved_MB_model=round(moved / 1e6, 2), launches=stage_times(lambda: F.marching_cubes(field)))
        if n_fields == 1:
            t0 = time.perf_counter()
            mo.marching_cubes(field.cpu().numpy(), dtype=np.float32)
            rec["cpu_oracle_numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            rec["cpu_threads"] = torch.get_num_threads()
        emit_line(rec)
    lab = torch.zeros(256, 256, 320, dtype=torch.int32, device=dev)
    zz, yy, xx = torch.meshgrid(torch.arange(256, device=dev), torch.arange(256, device=dev), torch.arange(320, device=dev), indexing="ij")
    for lb, (cz, cy, cx) in enumerate([(80, 80, 90), (80, 170, 90), (170, 80, 90), (128, 100, 230), (128, 180, 230)], 1):
        lab[((zz - cz) ** 2 + (yy - cy) ** 2 + ((xx - cx) * 0.8) ** 2) < 40 ** 2] = lb
    del zz, yy, xx
    v, f, n, nv, nf = F.marching_cubes_labels(lab, 1, 5)
    us, peak = measure(lambda: F.marching_cubes_labels(lab, 1, 5))
    out_bytes = v.numel() * 8 + f.numel() * 8
    emit_line(dict(kernel="mc marching_cubes_labels (count + host read + emit)", labels=5, shape=[256, 256, 320], hip_us=us,
                   hip_peak_MiB=peak, verts=sum(nv), faces=sum(nf), compulsory_MB=round((lab.numel() * 4 + out_bytes) / 1e6, 2),
                   launches=stage_times(lambda: F.marching_cubes_labels(lab, 1, 5))))
    del lab
    for B, C in [(8, 3), (1, 3)]:
        m = do.softmesh_case(B=B, K=C + 1, N=N)
        lg, xc = m["logits"].to(dev).requires_grad_(True), m["coords"].to(dev)
        gf = torch.randn(B * C, *res, device=dev)
        sm = SoftMesh(10, res, sig).to(dev)

        def meshes_fb():
            mm = sm.meshes(lg, xc)
            return torch.autograd.grad(mm.verts_packed().square().sum(), lg)
        psr_us, psr_peak = measure(lambda: torch.autograd.grad(sm.psr_grid(lg, xc), lg, gf), 5)
        mesh_us, mesh_peak = measure(meshes_fb, 5)
        rec = dict(kernel="mc SoftMesh.meshes fwd+bwd beside SoftMesh.psr_grid fwd+bwd", B=B, C=C, N=N, res=128, psr_grid_us=psr_us,
                   psr_grid_peak_MiB=psr_peak, meshes_us=mesh_us, meshes_peak_MiB=mesh_peak,
                   marching_cubes_share=round((mesh_us - psr_us) / mesh_us, 3))
        if mesh_us - psr_us > psr_us:
            rec["note"] = "THE MARCHING-CUBES STAGE IS SLOWER THAN THE WHOLE PSR FRONT"
        emit_line(rec)
    out_path = os.environ.get("FSG_MC_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "normals" in which:
    # point-cloud normals (csrc/pcl_normals.hip) at the DPSR workload's shape: 8 x 2048 points, three foreground labels and the
    # background by random assignment, packed by (item, label) as DPSRNet packs them, K = 30, grids of 128^3.  Four figures:
    # knn_segment alone, the normals kernel alone (the neighbour lists given), the same step as a torch composition on the device
    # (gather, einsum covariance, torch.linalg.eigh, the sign rule) -- the baseline, there is no earlier kernel --, and
    # DPSRNet.generate_meshes batched beside a Python loop over the (item, label) groups built from the same functions.  Each pair
    # is timed twice, alternating (HIP events, median of 30 after 5 warm-up calls), so the spread between rounds is on record.
    import json
    import numpy as np
    import normals_oracle as no
    from fissure_segmentation_amd.mesh import Meshes, join_meshes_as_batch
    from fissure_segmentation_amd.models.dpsr_net import DPSRNet, NORMALS_NEIGHBOURHOOD as K
    from fissure_segmentation_amd.models.dpsr_utils import differentiable_marching_cubes

    lines = []

    def emit_line(rec):
        print("NORMALS " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    def rounds(fn, iters=30, warm=5):
        return round(timeit(fn, iters, warm)[0], 1)

    B, N, C, res = 8, 2048, 4, (128, 128, 128)
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(np.stack([no.ellipsoid(N, 0.005, seed=50 + b).T for b in range(B)])).to(dev)      # (B, 3, N)
    label = torch.from_numpy(rng.integers(0, C, (B, N))).to(dev)
    logits = 10.0 * torch.nn.functional.one_hot(label, C).permute(0, 2, 1).float()
    groups = B * (C - 1)
    item = torch.arange(B, device=dev).view(B, 1)
    key = torch.where(label > 0, item * (C - 1) + label - 1, groups + item).reshape(-1)
    skey, perm = torch.sort(key, stable=True)
    ends = torch.bincount(key, minlength=groups + B).cumsum(0).to(torch.int32)
    pts = coords.transpose(1, 2).reshape(B * N, 3)[perm].contiguous()
    idx, _ = F.knn_segment(K, pts, pts, ends, ends)
    shape = dict(B=B, N=N, labels=C - 1, segments=groups + B, K=K)

    def kernel():
        return F._pcl_normals_raw(pts, ends, K, True, idx, True)

    def torch_form():
        nb = pts[idx.long()]
        c = nb - nb.mean(1, keepdim=True)
        w, V = torch.linalg.eigh(torch.einsum("nki,nkj->nij", c, c) / K)
        d = nb - pts[:, None]
        out = []
        for col in (0, 2):
            v = V[:, :, col]
            flip = ((v[:, None] * d).sum(-1) > 0).sum(1) < 0.5 * K
            out.append(torch.where(flip[:, None], -v, v))
        return w, torch.stack([out[0], torch.linalg.cross(out[1], out[0]), out[1]], -1)

    n_hip, w_hip, _ = kernel()
    w_t, f_t = torch_form()
    agree = float(((n_hip * f_t[:, :, 0]).sum(1).abs() > 0.999).float().mean())
    rec = dict(kernel="normals knn_segment alone", **shape)
    rec["hip_us"] = [rounds(lambda: F.knn_segment(K, pts, pts, ends, ends)) for _ in range(2)]
    emit_line(rec)
    rec = dict(kernel="normals kernel alone vs torch composition (gather, einsum, linalg.eigh, sign rule)", **shape)
    rec["hip_us"], rec["torch_us"] = [], []
    for _ in range(2):
        rec["hip_us"].append(rounds(kernel))
        rec["torch_us"].append(rounds(torch_form, 10, 2))
    rec["speedup"] = round(min(rec["torch_us"]) / max(rec["hip_us"]), 2)
    rec["normals_parallel_to_torch_share"] = round(agree, 4)
    rec["curvature_max_abs_diff"] = float((w_hip - w_t).abs().max())
    emit_line(rec)

    net = DPSRNet("DGCNN", k=20, in_features=3, num_classes=C, dpsr_res=res).to(dev).eval()

    def batched():
        return net.generate_meshes(coords, logits)

    def looped():       # the reference's loop (dpsr_net.py:145-165) over the same functions
        lab = logits.argmax(1)
        meshes = []
        for b in range(B):
            for lb in range(1, C):
                cur = coords[b, :, lab[b] == lb].transpose(-1, -2)
                if cur.shape[-2] < 3:
                    meshes.append(Meshes([cur.new_zeros(0, 3)], [torch.zeros(0, 3, dtype=torch.int64, device=dev)]))
                    continue
                v, f, n, nv, nf = differentiable_marching_cubes(net.compute_psr_grid(cur.unsqueeze(0)))
                meshes.append(Meshes([v[0, :nv[0]]], [f[0, :nf[0]]], [n[0, :nv[0]]]))
        return join_meshes_as_batch(meshes)

    with torch.no_grad():
        mb, ml = batched(), looped()
        rec = dict(kernel="normals DPSRNet.generate_meshes batched vs per-group loop", res=128, **shape)
        rec["verts_batched"], rec["verts_looped"] = int(mb.verts_packed().shape[0]), int(ml.verts_packed().shape[0])
        rec["batched_us"], rec["looped_us"] = [], []
        for _ in range(2):
            rec["batched_us"].append(rounds(batched, 5, 2))
            rec["looped_us"].append(rounds(looped, 5, 2))
        rec["speedup"] = round(min(rec["looped_us"]) / max(rec["batched_us"]), 2)
        emit_line(rec)
        fsg._lib.start_timing()
        for _ in range(5):
            batched()
        for name, t in fsg._lib.stop_timing().items():
            emit_line(dict(kernel="normals generate_meshes batched: " + name, calls_per_step=len(t) // 5,
                           median_us=round(1e3 * sorted(t)[len(t) // 2], 1)))
    out_path = os.environ.get("FSG_NORMALS_BENCH_OUT")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
if "surffit" in which:
    # surface fitting (csrc/mesh_cleanup.hip): consistent normal orientation, mesh clean-up and the whole fit_label_surfaces, each
    # beside a HOST baseline measured in the same run on the same graphs -- scipy.sparse.csgraph's minimum_spanning_tree /
    # breadth_first_order / connected_components plus numpy (tests/surface_fit_oracle.py); torch has no composition for either
    # graph problem, so there is no device column.  Device figures are HIP-event medians (whole call, its launches and plumbing
    # included), host figures wall clock.  The whole fit has no host counterpart (open3d is not installed): beside it stand the host
    # figures of its two graph steps on the same data.
    import json
    import time
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import breadth_first_order, connected_components, minimum_spanning_tree
    import surface_fit_oracle as so
    from fissure_segmentation_amd.data_processing import pointcloud_surface_fitting as sf
    from fissure_segmentation_amd.mesh import Meshes
    from fissure_segmentation_amd.utils import general_utils as gu

    lines = []

    def emit_line(rec):
        print("SURFFIT " + json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return round(statistics.median(ts), 1), out

    def host_orient(xyz, normals, idx, off):
        """scipy's minimum spanning tree of the same graph (integer weights 1 + the key's weight bits), a breadth-first walk per
        component for the signs, the root rule"""
        n = len(xyz)
        u, v, _, wb, _ = so.graph_edges(normals, idx, off)
        mst = minimum_spanning_tree(coo_matrix(((wb + 1).astype(np.float64), (u, v)), shape=(n, n)).tocsr())
        ncomp, lab = connected_components(mst, directed=False)
        signs = np.zeros(n, np.int8)
        for c in range(ncomp):
            members = np.nonzero(lab == c)[0]
            z = xyz[members, 2]
            top = int(members[np.nonzero(z == z.max())[0][0]])
            order, pred = breadth_first_order(mst, top, directed=False)
            flip = so.dot32(normals, order[1:], pred[order[1:]]) < 0
            par = np.zeros(n, bool)
            for node, p, f in zip(order[1:].tolist(), pred[order[1:]].tolist(), flip.tolist()):
                par[node] = par[p] ^ f
            s0 = -1 if normals[top, 2] < 0 else 1
            signs[order] = np.where(par[order], -s0, s0)
        return signs, ncomp

    K = 64
    for segments in (1, 3):
        parts = [so.ellipsoid(20000, 30 + s)[0] + np.float32(3 * s) for s in range(segments)]
        xyz, off = np.concatenate(parts), (np.arange(1, segments + 1) * 20000).astype(np.int32)
        x, o = torch.from_numpy(xyz).to(dev), torch.from_numpy(off).to(dev)
        idx = F.knn_segment(K, x, x, o, o)[0]
        normals = F._pcl_packed(x, o, 30, False, None, False, False)[0]
        med, mn = timeit(lambda: F.orient_normals_consistent(x, normals, o, K, idx=idx), iters=20, warm=3)
        out, signs, comp = F.orient_normals_consistent(x, normals, o, K, idx=idx)
        nh, ih = normals.cpu().numpy(), idx.cpu().numpy()
        t0 = time.perf_counter()
        hs, ncomp = host_orient(xyz, nh, ih, off)
        host_us = (time.perf_counter() - t0) * 1e6
        rec = dict(kernel="surffit orient_normals_consistent", segments=segments, points=len(xyz), K=K, hip_us=round(med, 1),
                   hip_min_us=round(mn, 1), knn_segment_us=round(timeit(lambda: F.knn_segment(K, x, x, o, o), 10, 2)[0], 1),
                   host_scipy_us=round(host_us, 1), speedup_vs_host=round(host_us / med, 1), components=int(ncomp),
                   components_hip=int(comp.unique().numel()), flipped=int((signs < 0).sum()),
                   signs_equal_host_share=round(float((signs.cpu().numpy() == hs).mean()), 6))
        if segments == 1:      # the exact oracle (Kruskal in the kernel's key order, a Python loop): equality, not a time
            t0 = time.perf_counter()
            want = so.orient(xyz, nh, ih, off)
            rec["oracle_kruskal_python_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            rec["signs_equal_oracle"] = bool(np.array_equal(signs.cpu().numpy(), want["signs"]))
            rec["components_equal_oracle"] = bool(np.array_equal(comp.cpu().numpy(), want["comp"]))
        fsg._lib.start_timing()
        for _ in range(5):
            F.orient_normals_consistent(x, normals, o, K, idx=idx)
        rec["entry_us"] = {k: round(1e3 * sorted(v)[len(v) // 2], 1) for k, v in fsg._lib.stop_timing().items()}
        emit_line(rec)

    # clean-up: three marching-cubes meshes of about 50 000 faces each (a big sphere and some small blobs per field)
    res = 128
    zz, yy, xx = np.meshgrid(*(np.arange(res, dtype=np.float32),) * 3, indexing="ij")
    fields = []
    for s in range(3):
        rng = np.random.default_rng(40 + s)
        f = np.sqrt((zz - 64) ** 2 + (yy - 64) ** 2 + (xx - 60 - 4 * s) ** 2) - 44
        for _ in range(6):
            c = rng.uniform(8, 120, 3)
            c[rng.integers(3)] = rng.choice([6.0, 121.0])          # near a wall of the volume: away from the sphere
            f = np.minimum(f, np.sqrt((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) - rng.uniform(2, 4.5))
        fields.append(f)
    field = torch.from_numpy(np.stack(fields)).to(dev)
    verts, faces, vnormals, nv, nf = F.marching_cubes(field, 0.0, return_local_coords=False)
    cut = lambda t, n: list(torch.split(t, n))                      # noqa: E731
    meshes = Meshes(cut(verts, nv), cut(faces, nf), cut(vnormals, nv))
    clusters, counts = F.mesh_face_components(meshes)
    rec = dict(kernel="surffit mesh clean-up", meshes=3, faces=nf, verts=nv, clusters=counts.tolist())
    for name, fn in (("face_components", lambda: F.mesh_face_components(meshes)),
                     ("component_stats", lambda: F.mesh_component_stats(meshes, clusters)),
                     ("remove_all_but_biggest_component", lambda: gu.remove_all_but_biggest_component(meshes, right=True, center_x=64.0))):
        rec[name + "_hip_us"] = round(timeit(fn, iters=10, warm=2)[0], 1)
    host = [(v.cpu().numpy(), f.cpu().numpy()) for v, f in zip(meshes.verts_list(), meshes.faces_list())]
    t0 = time.perf_counter()
    hc = [so.face_clusters(f) for _, f in host]
    t1 = time.perf_counter()
    hstats = [so.cluster_stats(v, f, c[0]) for (v, f), c in zip(host, hc)]
    t2 = time.perf_counter()
    hbig = []
    for v, f in host:
        k, cl, _ = so.biggest_component(v, f, True, 64.0)
        hbig.append(so.compact(v, f, np.ones(len(v), bool), cl == k, True))
    t3 = time.perf_counter()
    rec.update(face_components_host_scipy_us=round((t1 - t0) * 1e6, 1), component_stats_host_numpy_us=round((t2 - t1) * 1e6, 1),
               remove_all_but_biggest_component_host_us=round((t3 - t2) * 1e6, 1))
    got = gu.remove_all_but_biggest_component(meshes, right=True, center_x=64.0)
    rec["clusters_equal_host"] = bool(np.array_equal(clusters.cpu().numpy(), np.concatenate([c[0] for c in hc])))
    rec["biggest_equal_host"] = all(np.array_equal(g.cpu().numpy(), h[1]) for g, h in zip(got.faces_list(), hbig))
    area = F.mesh_component_stats(meshes, clusters)[0].cpu().numpy()
    rec["area_max_rel_diff_host_fp64"] = float(np.max(np.abs(area - np.concatenate([h[0] for h in hstats])) / np.concatenate([h[0] for h in hstats])))
    emit_line(rec)

    # the whole fit: three labels of 20 000 points each
    pts = np.concatenate([so.ellipsoid(20000, 50 + s)[0] * np.float32(40 + 5 * s) + np.float32(100 + 30 * s) for s in range(3)])
    labels = np.repeat(np.arange(1, 4), 20000)
    p, lab = torch.from_numpy(pts).to(dev), torch.from_numpy(labels).to(dev)
    for depth in (6, 7):
        sf.fit_label_surfaces(p, lab, 3, depth=depth, crop_to_bbox=True)
        us, out = wall(lambda: sf.fit_label_surfaces(p, lab, 3, depth=depth, crop_to_bbox=True))
        us_clean, _ = wall(lambda: gu.remove_all_but_biggest_component(out))
        emit_line(dict(kernel="surffit fit_label_surfaces (3 labels x 20000 points, crop)", depth=depth, hip_wall_us=us,
                       remove_all_but_biggest_component_wall_us=us_clean, verts=out._nv, faces=out._nf,
                       note="no host pipeline to race (open3d absent); the host figures of its graph steps are on the lines above"))
    out_path = os.environ.get("FSG_SURFFIT_BENCH_OUT", os.path.join(ROOT, "profiles", "surface_fit_bench.jsonl"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
if "reg" in which:
    # Dense Adam registration (csrc/dense_reg.hip, shape_model/adam_registration.py): one fused iteration (4 entry points) and a
    # 50-iteration run captured into one graph, beside the torch composition of the same loop (tests/reg_oracle.adam_loop, fp32,
    # on the device) in the same process, alternating; peak extra memory of both.  Writes profiles/reg_bench.jsonl.
    import json
    import reg_oracle as ro
    from fissure_segmentation_amd.shape_model import adam_registration as ar
    lines = []

    def emit_line(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 1)

    C, ITERS = 22, 50
    for (S, B) in [((64, 64, 64), 1), ((64, 64, 64), 4), ((96, 96, 104), 1), ((96, 96, 104), 4)]:
        g = torch.Generator(device=dev).manual_seed(7)
        ff = ro.smooth3(torch.rand(B, C, *S, device=dev, generator=g))
        ff = ((ff - ff.amin()) / (ff.amax() - ff.amin())).half().float()
        fm = torch.roll(ff, (1, -1, 1), (2, 3, 4))
        pf, pm = F.reg_pack_features(ff), F.reg_pack_features(fm)
        run = ar.InstanceOptimisation(pf, pm, C, iters=ITERS)
        run.iterate()                                              # loads the kernels; the parameter has left its start
        fused_it = timeit(lambda: run.iterate(0, 1), iters=40, warm=5)
        graph_run = ar.InstanceOptimisation(pf, pm, C, iters=ITERS)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graph_run.iterate()
        fused_50 = timeit(graph.replay, iters=10, warm=2)
        fused_50_eager = timeit(run.iterate, iters=10, warm=2)
        comp_it = timeit(lambda: ro.adam_loop(ff, fm, 1), iters=10, warm=2)      # (includes building Adam's state: one iteration)
        comp_50 = timeit(lambda: ro.adam_loop(ff, fm, ITERS), iters=4, warm=1)
        fused_50b = timeit(graph.replay, iters=10, warm=2)                       # again, after the composition: the spread
        fsg._lib.start_timing()
        for _ in range(10):
            run.iterate(0, 1)
        entry = {k: round(1e3 * sorted(v)[len(v) // 2], 1) for k, v in fsg._lib.stop_timing().items()}
        mem_fused = peak_extra(lambda: ar.adam_instance_optimisation(pf, pm, iters=ITERS, channels=C))
        mem_comp = peak_extra(lambda: ro.adam_loop(ff, fm, ITERS))
        fresh = ar.adam_instance_optimisation(pf, pm, iters=ITERS, channels=C)[1]      # (the timed runs went on from where they were)
        fused_first, fused_final = float(fresh[0].sum()), float(fresh[-1].sum())
        comp_final = float(ro.adam_loop(ff, fm, ITERS)[1][-1].sum())
        emit_line(dict(kernel="reg adam_instance_optimisation", grid=list(S), C=C, B=B, iters=ITERS,
                       fused_iteration_us=round(fused_it[0], 1), fused_iteration_min_us=round(fused_it[1], 1), entry_us=entry,
                       fused_50_graph_us=round(fused_50[0], 1), fused_50_graph_again_us=round(fused_50b[0], 1),
                       fused_50_eager_us=round(fused_50_eager[0], 1),
                       composition_1_iteration_us=round(comp_it[0], 1), composition_50_us=round(comp_50[0], 1),
                       speedup_50=round(comp_50[0] / fused_50[0], 2),
                       fused_peak_extra_MiB=mem_fused, composition_peak_extra_MiB=mem_comp,
                       final_objective_fused=fused_final, final_objective_composition=comp_final,
                       initial_objective=fused_first))
        del run, graph_run, graph
    out_path = os.environ.get("FSG_REG_BENCH_OUT", os.path.join(ROOT, "profiles", "reg_bench.jsonl"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
if "spatial" in which:
    # Voxel patch augmentation (csrc/spatial.hip): the prefilter, the elastic field, the fused resample at orders 3 and 1 and the
    # whole image_augmentation, volume 224 x 160 x 224, patch 128^3, B = 1 and 4.  The order-1 path (elastic field + resample of
    # image and labels) races the torch composition of the same math on the device in the same run, alternating (separable
    # conv3d smoothing + grid_sample; torch has no order-3 sampler); scipy on the host, the code batchgenerators calls, is the
    # other column (B = 1 item; FSG_SPATIAL_HOST=0 leaves it out).  Writes profiles/spatial_bench.jsonl.
    import json, time
    import numpy as np
    import spatial_oracle as so
    from fissure_segmentation_amd import augmentations as aug
    from torch.nn import functional as TF
    lines = []
    VOL, PATCH, SIGMA, ALPHA = (224, 160, 224), (128, 128, 128), 11.5, 500.0
    with_host = os.environ.get("FSG_SPATIAL_HOST", "1") != "0"

    def peak_extra(fn):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn(); torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 1)

    def composition(vol, seg, noise, matrix, centre, mirror, intensity):
        """the order-1 path in torch ops: zero-padded separable Gaussian (scipy's taps), coordinates, grid_sample (bilinear +
        border for the image, nearest + zeros for the labels), flips, intensity"""
        B = vol.shape[0]
        r = int(4 * SIGMA + 0.5)
        x = torch.arange(-r, r + 1, device=dev, dtype=torch.float32)
        w = torch.exp(-0.5 / SIGMA ** 2 * x * x)
        w = w / w.sum()
        e = noise.reshape(B * 3, 1, *PATCH)
        e = TF.conv3d(e, w.view(1, 1, 1, 1, -1), padding=(0, 0, r))
        e = TF.conv3d(e, w.view(1, 1, 1, -1, 1), padding=(0, r, 0))
        e = TF.conv3d(e, w.view(1, 1, -1, 1, 1), padding=(r, 0, 0))
        e = e.reshape(B, 3, *PATCH) * ALPHA
        grid = torch.stack(torch.meshgrid(*(torch.arange(p, device=dev, dtype=torch.float32) - (p - 1) / 2 for p in PATCH),
                                          indexing="ij"))
        src = torch.einsum("bij,bjdhw->bidhw", matrix, grid[None] + e) + centre[:, :, None, None, None]
        size = torch.tensor(VOL, device=dev, dtype=torch.float32).view(1, 3, 1, 1, 1)
        g = (2 * src / (size - 1) - 1).permute(0, 2, 3, 4, 1).flip(-1)
        img = TF.grid_sample(vol, g, mode="bilinear", padding_mode="border", align_corners=True)
        lab = TF.grid_sample(seg.float(), g, mode="nearest", padding_mode="zeros", align_corners=True).long()
        img = img * intensity[0] + intensity[1]
        outs = []
        for t in (img, lab):
            for ax in range(3):
                t = torch.where(mirror[:, ax].view(B, 1, 1, 1, 1), t.flip(2 + ax), t)
            outs.append(t)
        return outs

    for B in (1, 4):
        g = torch.Generator(device=dev).manual_seed(3)
        vol = torch.randn(B, 1, *VOL, device=dev, generator=g)
        seg = (torch.rand(B, 1, *VOL, device=dev, generator=g) * 5).long()
        p = aug.random_spatial_parameters(B, VOL, PATCH, generator=g)
        noise = torch.rand(B, 3, *PATCH, device=dev, generator=g) * 2 - 1
        inten = (2.0 / 1624.0, 0.26)
        coef = F.bspline_prefilter(vol)
        el = F.elastic_field(noise, SIGMA, ALPHA)
        kw = dict(matrix=p["matrix"], centre=p["centre"], elastic=el, mirror=p["mirror"], intensity=inten)
        rec = dict(kernel="voxel patch augmentation", volume=list(VOL), patch=list(PATCH), B=B, sigma=SIGMA)
        rec["prefilter_us"] = round(timeit(lambda: F.bspline_prefilter(vol), iters=10, warm=2)[0], 1)
        rec["elastic_field_us"] = round(timeit(lambda: F.elastic_field(noise, SIGMA, ALPHA), iters=10, warm=2)[0], 1)
        rec["resample_order3_us"] = round(timeit(lambda: F.spatial_transform(coef, seg, PATCH, order_data=3, prefiltered=True, **kw),
                                                 iters=10, warm=2)[0], 1)
        rec["resample_order1_us"] = round(timeit(lambda: F.spatial_transform(vol, seg, PATCH, order_data=1, **kw), iters=10, warm=2)[0], 1)
        rec["resample_order1_labels1_us"] = round(timeit(lambda: F.spatial_transform(vol, seg, PATCH, order_data=1, order_seg=1, **kw),
                                                         iters=10, warm=2)[0], 1)
        rec["image_augmentation_cached_us"] = round(timeit(lambda: aug.image_augmentation(coef, seg, PATCH, generator=g, prefiltered=True,
                                                                                          intensity=inten), iters=10, warm=2)[0], 1)
        rec["image_augmentation_uncached_us"] = round(timeit(lambda: aug.image_augmentation(vol, seg, PATCH, generator=g, intensity=inten),
                                                             iters=10, warm=2)[0], 1)

        def fused1():
            e = F.elastic_field(noise, SIGMA, ALPHA)
            return F.spatial_transform(vol, seg, PATCH, p["matrix"], p["centre"], elastic=e, mirror=p["mirror"], order_data=1,
                                       intensity=inten)

        def comp1():
            return composition(vol, seg, noise, p["matrix"], p["centre"], p["mirror"], inten)
        a = timeit(fused1, iters=8, warm=2)[0]
        c = timeit(comp1, iters=8, warm=2)[0]
        a2 = timeit(fused1, iters=8, warm=2)[0]
        rec["order1_path_fused_us"], rec["order1_path_fused_again_us"], rec["order1_path_torch_us"] = round(a, 1), round(a2, 1), round(c, 1)
        rec["order1_path_speedup"] = round(c / max(a, a2), 2)
        rec["order1_path_verdict"] = "fused wins" if max(a, a2) < c else "fused LOSES"
        fi, fl = fused1()
        ci, cl = comp1()
        rec["order1_image_max_abs_diff_vs_torch"] = float((fi - ci).abs().max())
        rec["order1_labels_differing_share_vs_torch"] = float((fl != cl).double().mean())
        rec["prefilter_peak_extra_MiB"] = peak_extra(lambda: F.bspline_prefilter(vol))
        rec["elastic_field_peak_extra_MiB"] = peak_extra(lambda: F.elastic_field(noise, SIGMA, ALPHA))
        rec["image_augmentation_cached_peak_extra_MiB"] = peak_extra(
            lambda: aug.image_augmentation(coef, seg, PATCH, generator=g, prefiltered=True, intensity=inten))
        rec["order1_path_fused_peak_extra_MiB"], rec["order1_path_torch_peak_extra_MiB"] = peak_extra(fused1), peak_extra(comp1)
        if with_host and B == 1:
            from scipy import ndimage as ndi
            v, s, n = vol[0, 0].cpu().numpy().astype(np.float64), seg[0, 0].cpu().numpy(), noise[0].cpu().numpy().astype(np.float64)
            t0 = time.perf_counter(); sm = ndi.gaussian_filter(n[0], SIGMA, mode="constant", cval=0)
            rec["scipy_gaussian_one_component_us"] = round((time.perf_counter() - t0) * 1e6)
            coords = so.coordinates(p["matrix"][:1].cpu().numpy(), p["centre"][:1].cpu().numpy(), el[:1].cpu().numpy(), PATCH)[0]
            t0 = time.perf_counter(); w3 = ndi.map_coordinates(v, coords, order=3, mode="nearest")
            rec["scipy_map_coordinates_order3_us"] = round((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); w1 = ndi.map_coordinates(v, coords, order=1, mode="nearest")
            rec["scipy_map_coordinates_order1_us"] = round((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); ndi.map_coordinates(s, coords, order=0, mode="constant", cval=0)
            rec["scipy_map_coordinates_labels_us"] = round((time.perf_counter() - t0) * 1e6)
            rec["scipy_whole_sample_order3_us"] = (3 * rec["scipy_gaussian_one_component_us"] + rec["scipy_map_coordinates_order3_us"]
                                                   + rec["scipy_map_coordinates_labels_us"])
            plain = dict(kw, mirror=None, intensity=None)
            g3 = F.spatial_transform(coef[:1], None, PATCH, order_data=3, prefiltered=True, **{k: (t[:1] if torch.is_tensor(t) else t)
                                                                                               for k, t in plain.items()})[0]
            rec["order3_max_abs_err_vs_scipy"] = float(np.abs(g3[0, 0].cpu().numpy() - w3).max())
            rec["speedup_vs_scipy_whole_sample"] = round(rec["scipy_whole_sample_order3_us"] / rec["image_augmentation_cached_us"], 1)
            del sm, w1
        lines.append(json.dumps(rec))
        print("SPATIAL " + lines[-1], flush=True)
        del vol, seg, coef, el, noise
    out_path = os.environ.get("FSG_SPATIAL_BENCH_OUT", os.path.join(ROOT, "profiles", "spatial_bench.jsonl"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
if "kmeans" in which:
    # Batched k-means (csrc/kmeans.hip) and data_set_correspondences.  One iteration and a whole run at the reference's sizes
    # (pooled clouds of 100 / 1000 instances of 1024 points, K = 1024), beside, in the same run, the torch composition on the
    # device (functional.knn_segment with k = 1 for the assignment, index_add_ for the sums) and, on the host for item 0 only,
    # scipy.cluster.vq.kmeans2 and sklearn.cluster.k_means from the same centres (FSG_KMEANS_HOST=0 leaves the host out);
    # peak extra memory; final inertia of every path; a whole data_set_correspondences in both modes against the per-pair
    # loop of the same calls.  Writes profiles/kmeans_bench.jsonl.
    import json
    import time
    import numpy as np
    import kmeans_oracle as ko
    from fissure_segmentation_amd.shape_model import generate_corresponding_points as gcp
    lines = []
    HOST = os.environ.get("FSG_KMEANS_HOST", "1") != "0"

    def emit_line(rec):
        lines.append(json.dumps(rec))
        print("KMEANS " + lines[-1], flush=True)

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
            del keep
        return round(statistics.median(ts), 1)

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 1)

    def torch_step(pts, cen):
        """one Lloyd iteration out of existing device pieces: the segment kNN with k = 1, then index_add_ (float atomics)"""
        B, n, K = pts.shape[0], pts.shape[1], cen.shape[1]
        seg = torch.arange(1, B + 1, dtype=torch.int32, device=pts.device)
        idx, d2 = F.knn_segment(1, cen.reshape(B * K, 3), pts.reshape(B * n, 3), seg * K, seg * n)
        flat = idx.reshape(-1).long()
        sums = torch.zeros(B * K, 3, device=pts.device).index_add_(0, flat, pts.reshape(B * n, 3))
        cnt = torch.zeros(B * K, device=pts.device).index_add_(0, flat, torch.ones(B * n, device=pts.device))
        new = torch.where(cnt[:, None] > 0, sums / cnt[:, None].clamp_min(1), cen.reshape(B * K, 3)).view(B, K, 3)
        return new, d2.view(B, n).double().sum(1)

    def torch_run(pts, cen, iters):
        for _ in range(iters):
            cen, _ = torch_step(pts, cen)
        return cen, torch_step(pts, cen)[1]

    for (B, I, P) in [(3, 100, 1024), (5, 1000, 1024)]:
        n, K = I * P, P
        pts = torch.from_numpy(np.stack([ko.pooled(I, P, 40 + b) for b in range(B)])).to(dev)
        t_fps = wall(lambda: F.kmeans(pts, K, max_iter=0), reps=1)
        c0 = F.kmeans(pts, K, max_iter=0)[0]
        print(f"KMEANS B={B} n={n} K={K}: farthest point sampling + one assign {t_fps} us", flush=True)
        step_us = timeit(lambda: F.kmeans_step(pts, c0), iters=10, warm=2)
        fsg._lib.start_timing()
        for _ in range(5):
            F.kmeans_step(pts, c0)
        entry = {k: round(1e3 * sorted(v)[len(v) // 2], 1) for k, v in fsg._lib.stop_timing().items()}
        comp_step_us = timeit(lambda: torch_step(pts, c0), iters=5, warm=1)
        cen, lab, inertia, n_iter = F.kmeans(pts, init=c0)
        iters = int(n_iter.max())
        run_us = wall(lambda: F.kmeans(pts, init=c0), reps=3)
        comp_run_us = wall(lambda: torch_run(pts, c0, iters), reps=1)
        comp_inertia = torch_run(pts, c0, iters)[1]
        rec = dict(kernel="kmeans", B=B, n=n, K=K, fps_init_plus_assign_us=t_fps, step_us=round(step_us[0], 1),
                   step_min_us=round(step_us[1], 1), entry_us=entry, torch_composition_step_us=round(comp_step_us[0], 1),
                   iterations=n_iter.tolist(), run_us=run_us, torch_composition_run_same_iterations_us=comp_run_us,
                   peak_extra_MiB=peak_extra(lambda: F.kmeans(pts, init=c0)),
                   torch_composition_peak_extra_MiB=peak_extra(lambda: torch_run(pts, c0, 1)),
                   initial_inertia=F.kmeans_step(pts, c0)[3].tolist(), final_inertia=inertia.tolist(),
                   torch_composition_final_inertia=comp_inertia.tolist())
        if HOST:
            from scipy.cluster.vq import kmeans2, vq
            p0, h0 = pts[0].cpu().numpy().astype(np.float64), c0[0].cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            kmeans2(p0, h0, iter=2, minit="matrix", missing="warn")
            rec["scipy_kmeans2_iteration_us_item0"] = round((time.perf_counter() - t0) * 1e6 / 2, 1)
            print("KMEANS scipy done", flush=True)
            try:
                from sklearn.cluster import k_means
                t0 = time.perf_counter()
                sc, sl, si, sn = k_means(p0, n_clusters=K, init=h0, n_init=1, max_iter=iters, tol=1e-4, return_n_iter=True)
                rec.update(sklearn_run_us_item0=round((time.perf_counter() - t0) * 1e6, 1), sklearn_iterations_item0=int(sn),
                           sklearn_final_inertia_item0=float(si))
            except ImportError:
                rec["sklearn"] = "not installed"
        emit_line(rec)
        del pts, c0, cen, lab

    inp = ko.correspondence_inputs(seed=77, instances=100, objects=2, P=1024, grid=32)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    args = lambda: (t(inp["fixed_pcs"]), inp["meshes"], t(inp["moving_pcs"]), [dict(d) for d in inp["transforms"]],   # noqa: E731
                    t(inp["moved_pcs"]), t(inp["displacements"]), None, None)

    def per_pair(mode):
        """the reference's double loop over the same public calls: one object and one instance at a time"""
        fixed, meshes, moving, tr, moved, disp = args()[:6]
        s, R, tl = gcp._transforms(tr, len(tr), dev)
        O, I = fixed.shape[0], moved.shape[0]
        cen = fixed if mode == "simple" else torch.stack(
            [F.kmeans(moved[:, o].reshape(-1, 3), n_clusters=fixed.shape[1])[0].double() for o in range(O)])
        return [gcp.object_correspondences(cen[o], moved[i:i + 1, o], disp[i:i + 1, o], moving[i:i + 1, o], [meshes[i][o]],
                                           s[i:i + 1], R[i:i + 1], tl[i:i + 1]) for o in range(O) for i in range(I)]

    for mode in ("simple", "kmeans"):
        gcp.data_set_correspondences(*args(), mode=mode, show=False)
        batched = wall(lambda: gcp.data_set_correspondences(*args(), mode=mode, show=False), reps=3)
        looped = wall(lambda: per_pair(mode), reps=2)
        emit_line(dict(kernel="data_set_correspondences", mode=mode, instances=100, objects=2, points=1024, mesh_faces=2 * 31 * 31,
                       batched_us=batched, per_pair_loop_us=looped, speedup=round(looped / batched, 2),
                       peak_extra_MiB=peak_extra(lambda: gcp.data_set_correspondences(*args(), mode=mode, show=False))))
    out_path = os.environ.get("FSG_KMEANS_BENCH_OUT", os.path.join(ROOT, "profiles", "kmeans_bench.jsonl"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
if "poisson" in which:
    # Weighted sample elimination (csrc/poisson_disk.hip) at the reference's size, N = 1024 points from M = 5 N uniform samples
    # of a unit square with open3d's radii, for B = 1, 8 and 256 items; beside it, in the same run, a torch composition of the
    # same rule on the device (the dense quantised pair matrix, built item by item into int32, and a host-free loop of
    # M - N rounds: key maximum, row gather, subtraction) and, on the host for item 0, the heap / KD-tree implementation
    # (tests/poisson_disk_oracle.eliminate_heap) and the numpy restatement; peak extra memory; whether the three agree with the
    # kernel.  Writes profiles/poisson_disk_bench.jsonl.
    import json
    import time
    import numpy as np
    import poisson_disk_oracle as po
    lines = []
    N, M = 1024, 5120

    def emit_line(rec):
        lines.append(json.dumps(rec))
        print("POISSON " + lines[-1], flush=True)

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
            del keep
        return round(statistics.median(ts), 1)

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 1)

    def torch_elimination(pts, n_keep, R, r_min):
        """the rule of the kernel out of torch operations: -> (keep (B, n_keep) ascending, order (B, M - n_keep))"""
        B, m = pts.shape[0], pts.shape[1]
        Q = torch.empty(B, m, m, dtype=torch.int32, device=pts.device)
        eye = torch.eye(m, dtype=torch.bool, device=pts.device)
        for b in range(B):
            p = pts[b]
            dx, dy, dz = (p[:, None, c] - p[None, :, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            t = (1.0 - torch.maximum(d2.sqrt(), r_min[b]) / R[b]).clamp_min(0.0)
            t = t * t
            t = t * t
            t = t * t
            Q[b] = torch.where((d2 < R[b] * R[b]) & ~eye & (R[b] > 0), torch.round(t * 16777216.0), 0.0).to(torch.int32)
        w = Q.sum(2, dtype=torch.int64)
        rows = torch.arange(B, device=pts.device)
        low = (16383 - torch.arange(m, device=pts.device))[None]
        alive = torch.ones(B, m, dtype=torch.bool, device=pts.device)
        order = torch.empty(B, m - n_keep, dtype=torch.int64, device=pts.device)
        for r in range(m - n_keep):
            i = 16383 - torch.where(alive, w * 16384 + low, -1).amax(1) % 16384
            order[:, r] = i
            alive[rows, i] = False
            w -= Q[rows, i]
        return alive.nonzero()[:, 1].view(B, n_keep), order

    R0, r0 = po.radii(1.0, N, M)
    for B in (1, 8, 256):
        pts = torch.from_numpy(np.stack([po.unit_square(100 + b, M) for b in range(B)])).to(dev)
        R, r_min = torch.full((B,), float(R0), device=dev), torch.full((B,), float(r0), device=dev)
        keep, order = F.sample_elimination(pts, N, R, r_min, return_order=True)
        us = timeit(lambda: F.sample_elimination(pts, N, R, r_min, return_order=True), iters=7, warm=2)
        first = timeit(lambda: F.sample_elimination(pts, M - 1, R, r_min, return_order=True), iters=7, warm=2)
        rec = dict(kernel="sample_elimination", B=B, N=N, M=M, R=float(R0), r_min=float(r0), us=round(us[0], 1),
                   min_us=round(us[1], 1), us_per_round=round(us[0] / (M - N), 3),
                   weights_launch_plus_one_round_us=round(first[0], 1),
                   peak_extra_MiB=peak_extra(lambda: F.sample_elimination(pts, N, R, r_min, return_order=True)))
        ck, co = torch_elimination(pts, N, R, r_min)
        rec.update(torch_composition_equal=bool(torch.equal(ck, keep) and torch.equal(co, order)),
                   torch_composition_us=wall(lambda: torch_elimination(pts, N, R, r_min), reps=1 if B > 8 else 2),
                   torch_composition_peak_extra_MiB=peak_extra(lambda: torch_elimination(pts, N, R, r_min)))
        del ck, co
        p0 = pts[0].cpu().numpy()
        t0 = time.perf_counter()
        hk, ho = po.eliminate_heap(p0, N, R0, r0)
        rec["host_heap_kdtree_us_item0"] = round((time.perf_counter() - t0) * 1e6, 1)
        t0 = time.perf_counter()
        ak, ao = po.eliminate(p0, N, R0, r0)
        rec["host_numpy_restatement_us_item0"] = round((time.perf_counter() - t0) * 1e6, 1)
        rec["host_equal_item0"] = bool(np.array_equal(hk, keep[0].cpu().numpy()) and np.array_equal(ho, order[0].cpu().numpy())
                                       and np.array_equal(ak, hk) and np.array_equal(ao, ho))
        rec["min_nn_distance_over_R_item0"] = round(po.min_nn_distance(p0[hk]) / float(R0), 4)
        emit_line(rec)
        del pts, keep, order
    out_path = os.environ.get("FSG_POISSON_BENCH_OUT", os.path.join(ROOT, "profiles", "poisson_disk_bench.jsonl"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
if "dsegae" in which:
    # DSEG-AE (csrc/dseg_ae.hip, dseg_ae_regularization.py): a cloud of 32 768 points with three objects of about 3 000, 6 000 and
    # 12 000 points, n_points_ae = 2048, at B = 1 and B = 8.  (1) fps_start against functional.fps on the same segments, each
    # length alone and all together; (2) reconstruct_packed against the reference-shaped loop on the device (boolean masks, the
    # reference's pure-torch sampling loop, one auto-encoder call per object); (3) the partition and extension launches alone and
    # peak extra memory.  HIP-event medians of whole calls after warm-up, the two sides of a comparison alternating in one run,
    # with the spread (min .. max) of the repeats.  Appends to profiles/dseg_ae_bench.jsonl.
    import json
    import tempfile
    import numpy as np
    from golden_util import fill_state_dict
    from fissure_segmentation_amd.dseg_ae_regularization import RegularizedSegDGCNN
    from fissure_segmentation_amd.models.dgcnn import DGCNNSeg
    from fissure_segmentation_amd.models.folding_net import DGCNNFoldingNet
    lines = []
    N, N_AE, SIZES = 32768, 2048, (3000, 6000, 12000)

    def emit_line(rec):
        lines.append(json.dumps(rec))
        print("DSEGAE " + lines[-1], flush=True)

    def event_us(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); keep = fn(); e.record(); torch.cuda.synchronize()
        del keep
        return s.elapsed_time(e) * 1e3

    def alternate(sides, reps, warm=2):
        """{name: fn} -> {name: (median, min, max)} in us, the sides taking turns inside every repeat"""
        for _ in range(warm):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():
                ts[k].append(event_us(fn))
        return {k: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for k, v in ts.items()}

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 2)

    def labelled(seed, B, sizes):
        rng = np.random.default_rng(seed)
        x = torch.from_numpy(cloud(seed, B, 3, N)).to(dev)
        seg = np.zeros((B, N), np.int64)
        for b in range(B):
            perm, q = rng.permutation(N), 0
            for o, s in enumerate(sizes):
                n = int(s * rng.uniform(0.95, 1.05))
                seg[b, perm[q:q + n]] = o + 1
                q += n
        return x, torch.from_numpy(seg).to(dev)

    def reference_loop(model, x, seg):
        """per object: boolean mask, the oracle's restatement of the pure-torch sampling loop (oracle/ref_cpu.py: device tensors
        in, the index list on the host, so one arg-max round trip per sample) with a drawn start, one auto-encoder call"""
        from oracle import ref_cpu
        out = []
        for b in range(x.shape[0]):
            xb, sb = x[b:b + 1], seg[b:b + 1]
            for obj in range(1, model.seg_model.num_classes):
                pts = xb[:, :3].transpose(1, 2)[sb == obj].view(1, -1, 3)
                if pts.shape[1] < model.ae.encoder.k:
                    continue
                start = int(torch.randint(pts.shape[1], (1,)))
                sampled = ref_cpu.farthest_point_sampling(pts, model.n_points_ae, start)[0].transpose(1, 2)
                out.append(model.ae(sampled.contiguous()))
        return out

    with tempfile.TemporaryDirectory() as tmp:
        seg_net = fill_state_dict(DGCNNSeg(k=20, in_features=3, num_classes=4), 1)
        ae = fill_state_dict(DGCNNFoldingNet(k=20, n_embedding=512, shape_type='plane', n_input_points=N_AE, decode_mesh=True), 2)
        seg_net.save(os.path.join(tmp, "seg.pth"))
        ae.save(os.path.join(tmp, "ae.pth"))
        model = RegularizedSegDGCNN(os.path.join(tmp, "seg.pth"), os.path.join(tmp, "ae.pth"), n_points_seg=2048,
                                    n_points_ae=N_AE).to(dev).eval()
    for B in (1, 8):
        x, seg = labelled(50 + B, B, SIZES)
        counts, offset, xyz, src = F.label_partition(seg, x, 3)
        lens = counts.flatten().tolist()
        n = int(offset[-1])
        xyz = xyz[:n].contiguous()
        G_ = len(lens)
        new_off = torch.arange(1, G_ + 1, dtype=torch.int32, device=dev) * N_AE
        # (1) sampling: every length alone (item 0's three objects), then all groups in one call
        if B == 1:
            st = 0
            for ln in lens:
                one = xyz[st:st + ln].contiguous()
                o1 = torch.tensor([ln], dtype=torch.int32, device=dev)
                m1 = torch.tensor([N_AE], dtype=torch.int32, device=dev)
                assert torch.equal(F.fps_start(one, o1, m1, N_AE), F.fps(one, o1, m1, N_AE))
                r = alternate({"fps_start": lambda: F.fps_start(one, o1, m1, N_AE), "fps": lambda: F.fps(one, o1, m1, N_AE)}, reps=7)
                emit_line(dict(kernel="fps_start_vs_fps", segments=1, length=ln, samples=N_AE, fps_start_us=r["fps_start"],
                               fps_us=r["fps"], speedup=round(r["fps"][0] / r["fps_start"][0], 2), equal=True,
                               columns="median, min, max over 7 alternating repeats"))
                st += ln
        assert torch.equal(F.fps_start(xyz, offset, new_off, G_ * N_AE), F.fps(xyz, offset, new_off, G_ * N_AE))
        r = alternate({"fps_start": lambda: F.fps_start(xyz, offset, new_off, G_ * N_AE),
                       "fps": lambda: F.fps(xyz, offset, new_off, G_ * N_AE)}, reps=7)
        emit_line(dict(kernel="fps_start_vs_fps", B=B, segments=G_, lengths=lens, samples=N_AE, fps_start_us=r["fps_start"],
                       fps_us=r["fps"], speedup=round(r["fps"][0] / r["fps_start"][0], 2), equal=True,
                       columns="median, min, max over 7 alternating repeats"))
        # (2) the pipeline after the segmentation
        with torch.no_grad():
            r = alternate({"packed": lambda: model.reconstruct_packed(x, seg), "loop": lambda: reference_loop(model, x, seg)},
                          reps=3, warm=1)
            emit_line(dict(kernel="reconstruct_packed_vs_reference_loop", B=B, N=N, lengths=lens, n_points_ae=N_AE,
                           ae="k=20, n_embedding=512, folding decoder, m=2025", packed_us=r["packed"], loop_us=r["loop"],
                           speedup=round(r["loop"][0] / r["packed"][0], 2),
                           packed_peak_extra_MiB=peak_extra(lambda: model.reconstruct_packed(x, seg)),
                           loop_peak_extra_MiB=peak_extra(lambda: reference_loop(model, x, seg)),
                           columns="median, min, max over 3 alternating repeats"))
        # (3) the partition alone, against the boolean masks it replaces; the extension on objects shorter than n_points_ae
        masks = lambda: [x[b:b + 1, :3].transpose(1, 2)[seg[b:b + 1] == o] for b in range(B) for o in (1, 2, 3)]   # noqa: E731
        r = alternate({"partition": lambda: F.label_partition(seg, x, 3), "masks": masks}, reps=15)
        xs, ss = labelled(60 + B, B, (500, 1000, 1500))
        c2, o2, p2, _ = F.label_partition(ss, xs, 3)
        l2 = c2.flatten().tolist()
        p2 = p2[:int(o2[-1])].contiguous()
        P_ = sum(N_AE - v for v in l2)
        d_src = torch.cat([torch.randint(v, (N_AE - v,)) for v in l2]).to(dev)
        d_dir, d_z = torch.randn(P_, 3, device=dev), torch.randn(P_, device=dev)
        nn_d2 = F.knn_segment(2, p2, p2, o2, o2)[1][:, 1].contiguous()
        ends2 = o2.tolist()
        e = alternate({"extend_with_knn": lambda: F.segment_jitter_extend(p2, ends2, N_AE, d_src, d_dir, d_z),
                       "extend_given_nn": lambda: F.segment_jitter_extend(p2, ends2, N_AE, d_src, d_dir, d_z, nn_d2=nn_d2)}, reps=15)
        emit_line(dict(kernel="partition_and_extension", B=B, N=N, partition_us=r["partition"], boolean_masks_us=r["masks"],
                       partition_peak_extra_MiB=peak_extra(lambda: F.label_partition(seg, x, 3)),
                       boolean_masks_peak_extra_MiB=peak_extra(masks), extension_lengths=l2, extension_target=N_AE,
                       extension_with_knn_us=e["extend_with_knn"], extension_given_nn_us=e["extend_given_nn"],
                       extension_peak_extra_MiB=peak_extra(lambda: F.segment_jitter_extend(p2, ends2, N_AE, d_src, d_dir, d_z)),
                       columns="median, min, max over 15 alternating repeats (host-side wrapper included)"))
        # (4) random_extend: two objects shorter than n_points_ae beside a long one.  On: only the short groups are extended, one
        # auto-encoder forward; off: they go in at their own size, one forward per distinct size
        xm, sm = labelled(70 + B, B, (500, 1500, 12000))

        def packed_extend(flag):
            model.random_extend = flag
            try:
                return model.reconstruct_packed(xm, sm)
            finally:
                model.random_extend = False
        with torch.no_grad():
            r = alternate({"on": lambda: packed_extend(True), "off": lambda: packed_extend(False)}, reps=7)
        emit_line(dict(kernel="reconstruct_packed_random_extend", B=B, N=N, lengths=F.label_partition(sm, xm, 3)[0].flatten().tolist(),
                       n_points_ae=N_AE, random_extend_on_us=r["on"], random_extend_off_us=r["off"],
                       on_peak_extra_MiB=peak_extra(lambda: packed_extend(True)),
                       off_peak_extra_MiB=peak_extra(lambda: packed_extend(False)),
                       columns="median, min, max over 7 alternating repeats"))
    out_path = os.environ.get("FSG_DSEGAE_BENCH_OUT", os.path.join(ROOT, "profiles", "dseg_ae_bench.jsonl"))
    with open(out_path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
if "tps" in which:
    # Thin-plate-spline interpolation (csrc/tps.hip) at the workload's shape: B = 32 (instance, object) pairs, n = Q = 1024, image
    # 256 x 256 x 320.  The fit split into assembly and solve; the sparse route (functional.tps_grid_sample) and the whole
    # interpolate_displacements_tps; thin_plate_dense for ONE pair (a 251 MB field); and, in the same run, the reference-shaped
    # dense route for one pair as a torch composition on the device (fp32 fit with expanded distances, the lattice in chunks of
    # 4096, F.interpolate, F.grid_sample), with peak extra memory and what the routes differ by.  Writes profiles/tps_bench.jsonl.
    import json
    import numpy as np
    import tps_oracle as to
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    from fissure_segmentation_amd._launch import _p, launch
    lines = []

    def emit_line(rec):
        lines.append(json.dumps(rec))
        print("TPS " + lines[-1], flush=True)

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 1)

    def us(fn, iters=10, warm=2):
        med, mn = timeit(fn, iters=iters, warm=warm)
        return round(med, 1)

    B, n, Q, shape = 32, 1024, 1024, (320, 256, 256)   # img_shape = (D, H, W)
    D, H, W = shape
    cases = [to.voxel_case(shape, n, Q, 500 + b) for b in range(B)]
    e, v, q = (torch.from_numpy(np.stack([c[k] for c in cases])).to(dev) for k in range(3))
    norm = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float32, device=dev)
    control, values, grid = e / norm * 2 - 1, v / norm * 2, q / norm * 2 - 1
    size = (W, H, D)

    def u32(r):
        return r.square() * torch.log(r + 1e-6)

    def d32(a, b):
        return (a.square().sum(1)[:, None] + b.square().sum(1)[None, :] - 2.0 * (a @ b.t())).clamp_(min=0.0).sqrt()

    def dense_composition(c, f, g):
        """one pair, the reference's shape of the computation, fp32 on the device"""
        A = torch.zeros(n + 4, n + 4, device=dev)
        A[:n, :n] = u32(d32(c, c)) + to.LAMBDA * torch.eye(n, device=dev)
        A[:n, n] = A[n, :n] = 1.0
        A[:n, n + 1:] = c
        A[n + 1:, :n] = c.t()
        rhs = torch.zeros(n + 4, 3, device=dev)
        rhs[:n] = f
        theta = torch.linalg.solve(A, rhs)
        D1, H1, W1 = (s // to.STEP for s in size)
        x2 = torch.nn.functional.affine_grid(torch.eye(3, 4, device=dev)[None], (1, 1, D1, H1, W1), align_corners=True).view(-1, 3)
        y2 = torch.cat([u32(d32(x2[j:j + 4096], c)) @ theta[:n] + theta[n] + x2[j:j + 4096] @ theta[n + 1:]
                        for j in range(0, len(x2), 4096)])
        y2 = y2.view(1, D1, H1, W1, 3).permute(0, 4, 1, 2, 3)
        field = torch.nn.functional.interpolate(y2, size, mode="trilinear", align_corners=True)
        out = torch.nn.functional.grid_sample(field, g.view(1, -1, 1, 1, 3), align_corners=False)
        return out.reshape(3, -1).t()

    with torch.no_grad():
        A = F.tps_system(control, to.LAMBDA)
        rhs = torch.zeros(B, n + 4, 3, dtype=torch.float64, device=dev)
        rhs[:, :n] = values
        theta = F.tps_fit(control, values, to.LAMBDA)
        sparse = F.tps_grid_sample(grid, control, theta, size)
        rec = dict(kernel="tps", B=B, n=n, Q=Q, img_shape=list(shape), lattice=[s // to.STEP for s in size],
                   assembly_us=us(lambda: F.tps_system(control, to.LAMBDA)),
                   solve_us=us(lambda: torch.linalg.solve(A, rhs), iters=5, warm=1),
                   fit_us=us(lambda: F.tps_fit(control, values, to.LAMBDA), iters=5, warm=1),
                   grid_sample_us=us(lambda: F.tps_grid_sample(grid, control, theta, size)),
                   interpolate_displacements_tps_us=us(lambda: pcr.interpolate_displacements_tps(e, v, q, shape), iters=5, warm=1),
                   fit_peak_extra_MiB=peak_extra(lambda: F.tps_fit(control, values, to.LAMBDA)),
                   grid_sample_peak_extra_MiB=peak_extra(lambda: F.tps_grid_sample(grid, control, theta, size)))
        emit_line(rec)
        del A, rhs

        # the 'nullspace' solver (csrc/tps_nullspace.hip) beside 'lu': the two alternate call by call in this process, HIP-event
        # medians; the stages of the new route; one pair; peak extra memory; what the thetas and the sampled outputs differ by
        def alternate(fns, rounds=7, warm=1):
            """{name: median microseconds}, the calls taking turns"""
            ts = {k: [] for k in fns}
            for r in range(warm + rounds):
                for k, fn in fns.items():
                    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    keep = fn()
                    t.record()
                    torch.cuda.synchronize()
                    del keep
                    if r >= warm:
                        ts[k].append(s.elapsed_time(t) * 1e3)
            return {k: round(float(np.median(v)), 1) for k, v in ts.items()}

        fit = lambda solver, s=slice(None): F.tps_fit(control[s], values[s], to.LAMBDA, solver=solver)   # noqa: E731
        interp = lambda solver: pcr.interpolate_displacements_tps(e, v, q, shape, solver=solver)   # noqa: E731
        fit_us = alternate({k: (lambda k=k: fit(k)) for k in ("lu", "nullspace")})
        interp_us = alternate({k: (lambda k=k: interp(k)) for k in ("lu", "nullspace")})
        one_us = alternate({k: (lambda k=k: fit(k, slice(0, 1))) for k in ("lu", "nullspace")})
        V, tau, R, S, info = F.tps_nullspace_system(control, to.LAMBDA)
        L, _ = F.cholesky_factor(S)
        v64 = values.double().contiguous()
        work = torch.empty(B * n * 3 * fsg._lib.TPS_NS_SOLVE_WORK_PER_VALUE, dtype=torch.float64, device=dev)
        th_buf = torch.empty(B, n + 4, 3, dtype=torch.float64, device=dev)
        cc = control.contiguous()
        stage_us = dict(system_us=us(lambda: F.tps_nullspace_system(control, to.LAMBDA)),
                        factor_us=us(lambda: F.cholesky_factor(S)),
                        solve_us=us(lambda: launch(dev, "fsg_tps_ns_solve_f64", _p(cc), _p(v64), _p(V), _p(tau), _p(R), _p(L), B, n, 3,
                                                   to.LAMBDA, _p(work), _p(th_buf))))
        th_lu, th_ns = fit("lu"), fit("nullspace")
        out_lu, out_ns = interp("lu"), interp("nullspace")
        emit_line(dict(kernel="tps_nullspace", B=B, n=n, Q=Q, img_shape=list(shape),
                       fit_us=fit_us, interpolate_displacements_tps_us=interp_us, one_pair_fit_us=one_us, **stage_us,
                       fit_peak_extra_MiB={k: peak_extra(lambda k=k: fit(k)) for k in ("lu", "nullspace")},
                       status_nonzero=int((info != 0).sum()),
                       theta_apart=float((th_ns - th_lu).abs().max() / th_lu.abs().max()),
                       sampled_apart=float((out_ns - out_lu).abs().max() / out_lu.abs().max()),
                       note="microseconds, medians of HIP-event times, 'lu' and 'nullspace' alternating; factor_us includes the copy "
                            "of S that cholesky_factor makes without overwrite=True; *_apart relative to the largest entry"))
        del V, tau, R, S, L, work, th_buf, th_lu, th_ns
        one = lambda: pcr.thin_plate_dense(control[:1], values[:1], size, to.STEP, to.LAMBDA)   # noqa: E731
        lattice_us = us(lambda: F.tps_eval(tuple(s // to.STEP for s in size), control[:1], theta[:1]))
        comp = lambda: dense_composition(control[0], values[0], grid[0])   # noqa: E731
        field = one()
        via_field = torch.nn.functional.grid_sample(field.permute(0, 4, 1, 2, 3), grid[:1].view(1, -1, 1, 1, 3),
                                                    align_corners=False).reshape(3, -1).t()
        del field
        ref = comp()
        scale = float(sparse[0].abs().max())
        emit_line(dict(kernel="tps_one_pair", n=n, Q=Q, img_shape=list(shape),
                       sparse_route_fit_plus_sample_us=us(lambda: F.tps_grid_sample(grid[:1], control[:1], F.tps_fit(control[:1], values[:1], to.LAMBDA), size), iters=5, warm=1),
                       lattice_eval_us=lattice_us, thin_plate_dense_us=us(one, iters=5, warm=1),
                       reference_shaped_dense_route_us=us(comp, iters=5, warm=1),
                       thin_plate_dense_peak_extra_MiB=peak_extra(one), reference_shaped_dense_route_peak_extra_MiB=peak_extra(comp),
                       sparse_vs_thin_plate_dense_plus_grid_sample=float((sparse[0] - via_field).abs().max()) / scale,
                       sparse_vs_reference_shaped_fp32_route=float((sparse[0] - ref).abs().max()) / scale,
                       note="errors relative to the largest sampled displacement of the pair"))
    out_path = os.environ.get("FSG_TPS_BENCH_OUT", os.path.join(ROOT, "profiles", "tps_bench.jsonl"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
if "optics" in which:
    # OPTICS (csrc/optics.hip) at the reference's size: three pooled sheets of 100 instances x 1024 points (n = 102 400),
    # min_samples 6, max_eps = 5 % of the coordinate range.  Whole call (wall, synchronised), the host extraction (xi labels and
    # cluster means, shape_model/optics.py), peak extra memory, cluster and noise counts; beside it sklearn.cluster.OPTICS on
    # the host for ONE item of 32 x 256 = 8 192 points, and for one 102 400-point item only with FSG_OPTICS_HOST_LARGE=1.  The
    # times of the three launches come from torch's profiler, last, so that a failure there loses nothing.  Writes
    # profiles/optics_bench.jsonl.
    import json
    import time
    import numpy as np
    import optics_oracle as oo
    from fissure_segmentation_amd.shape_model.optics import cluster_means, optics_xi_labels
    lines = []
    out_path = os.environ.get("FSG_OPTICS_BENCH_OUT", os.path.join(ROOT, "profiles", "optics_bench.jsonl"))

    def flush_lines():
        with open(out_path, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in lines) + "\n")

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
            del keep
        return round(statistics.median(ts), 1)

    def extract(pts_host, out, k):
        """host part: square roots, xi labels and fp64 means per item -> (seconds, clusters, noise points)"""
        order, _, reach2, pred = [t.cpu().numpy() for t in out]
        t0 = time.perf_counter()
        clusters, noise = [], []
        for b in range(len(pts_host)):
            labels = optics_xi_labels(np.sqrt(reach2[b]), pred[b], order[b], k)
            cluster_means(pts_host[b], labels)
            clusters.append(int(labels.max()) + 1)
            noise.append(int((labels < 0).sum()))
        return time.perf_counter() - t0, clusters, noise

    def stages(fn):
        """device time of the three launches of one call, by kernel name, in microseconds"""
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        got = {}
        for ev in prof.events():
            for key in ("optics_cells", "optics_core", "optics_order"):
                if key in ev.name:
                    t = getattr(ev, "device_time_total", None)
                    got[key] = got.get(key, 0.0) + float(t if t is not None else getattr(ev, "cuda_time_total", 0.0))
        return {k: round(v, 1) for k, v in got.items()}

    k = 6
    records = []
    for (B, I, P) in [(1, 32, 256), (3, 100, 1024)]:
        n = I * P
        host = np.stack([oo.pooled(I, P, 60 + b) for b in range(B)])
        eps = [oo.heuristic_eps(h) for h in host]
        pts = torch.from_numpy(host).to(dev)
        e = torch.tensor(eps, dtype=torch.float64, device=dev)
        run = lambda pts=pts, e=e: F.optics(pts, k, e, return_squared=True)   # noqa: E731  (bound now: `stages` calls it later)
        out = run()
        torch.cuda.synchronize()
        call_us = wall(run, reps=3)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = run()
        torch.cuda.synchronize()
        peak = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        del keep
        host_s, clusters, noise = extract(host, out, k)
        rec = dict(kernel="optics", B=B, n=n, min_samples=k, max_eps=[round(x, 4) for x in eps], call_us=call_us,
                   call_us_per_point_of_one_item=round(call_us / n, 3), host_extraction_us=round(host_s * 1e6, 1),
                   peak_extra_MiB=peak, clusters=clusters, noise=noise, stage_us="not measured")
        if (n == 8192 or os.environ.get("FSG_OPTICS_HOST_LARGE") == "1"):
            try:
                from sklearn.cluster import OPTICS
                t0 = time.perf_counter()
                sk = OPTICS(min_samples=k, max_eps=eps[0]).fit(host[0].astype(np.float64))
                rec["sklearn_fit_us_item0"] = round((time.perf_counter() - t0) * 1e6, 1)
                ours = optics_xi_labels(np.sqrt(out[2][0].cpu().numpy()), out[3][0].cpu().numpy(), out[0][0].cpu().numpy(), k)
                rec["sklearn_same_ordering_item0"] = bool(np.array_equal(sk.ordering_, out[0][0].cpu().numpy()))
                rec["sklearn_same_labels_item0"] = bool(np.array_equal(sk.labels_, ours))
            except ImportError:
                rec["sklearn"] = "not installed"
        lines.append(rec)
        records.append((rec, run, n))
        print("OPTICS " + json.dumps(rec), flush=True)
        flush_lines()
    for rec, run, n in records:
        try:
            st = stages(run)
            if st:
                rec["stage_us"] = st
                if "optics_order" in st:
                    rec["ordering_us_per_step"] = round(st["optics_order"] / n, 3)
        except Exception as ex:   # the profiler is an extra: the record keeps "not measured"
            print("OPTICS profiler failed:", repr(ex), flush=True)
        print("OPTICS " + json.dumps(rec), flush=True)
        flush_lines()
if "chol" in which:
    # Batched fp64 Cholesky (csrc/cholesky.hip): factor + solve (r = 3) beside torch.linalg.solve_ex and torch.linalg.cholesky_ex +
    # torch.cholesky_solve on the same matrices; the CPD assembly kernel beside its torch composition; the whole 100-iteration
    # deformable run at B = 32, M = N = 1024 under both solvers; peak extra memory of each.  HIP-event medians, the sides of a
    # comparison alternating in one run.  Writes profiles/cholesky_bench.jsonl.
    import json
    import chol_oracle as co
    import cpd_oracle
    from fissure_segmentation_amd.shape_model import point_cloud_registration as pcr
    lines = []
    out_path = os.environ.get("FSG_CHOL_BENCH_OUT", os.path.join(ROOT, "profiles", "cholesky_bench.jsonl"))

    def emit_line(rec):
        lines.append(json.dumps(rec))
        print("CHOL " + lines[-1], flush=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def alternating(sides, iters, warm=1):
        """{name: fn} -> {name: median microseconds}, one call of every side per round"""
        for _ in range(warm):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in sides}
        for _ in range(iters):
            for name, fn in sides.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); fn(); e.record(); torch.cuda.synchronize()
                ts[name].append(s.elapsed_time(e) * 1e3)
        return {name: round(statistics.median(v), 1) for name, v in ts.items()}

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return round(peak / 2 ** 20, 1)

    with torch.no_grad():
        for (B, n) in [(1, 1024), (32, 1024), (32, 256), (8, 2048)]:
            g = torch.Generator(device=dev).manual_seed(n + B)
            Q = torch.randn(B, n, n + 8, generator=g, dtype=torch.float64, device=dev)
            A = Q @ Q.transpose(1, 2) / n + 0.01 * torch.eye(n, dtype=torch.float64, device=dev)
            A = torch.tril(A) + torch.tril(A, -1).transpose(1, 2)
            b = torch.randn(B, n, 3, generator=g, dtype=torch.float64, device=dev)
            del Q
            sides = {"ours_factor_plus_solve_us": lambda: F.spd_solve(A, b),
                     "torch_solve_ex_us": lambda: torch.linalg.solve_ex(A, b),
                     "torch_cholesky_ex_plus_cholesky_solve_us": lambda: torch.cholesky_solve(b, torch.linalg.cholesky_ex(A)[0])}
            rec = dict(kernel="cholesky", B=B, n=n, r=3, **alternating(sides, iters=7))
            L, info = F.cholesky_factor(A)
            rec.update(alternating({"ours_factor_us": lambda: F.cholesky_factor(A), "ours_solve_us": lambda: F.cholesky_solve(L, b)}, iters=7))
            X, Xt = F.cholesky_solve(L, b), torch.linalg.solve_ex(A, b)[0]
            rec["info_clean"] = not bool(info.any())
            rec["ours_vs_solve_ex_rel"] = float((X - Xt).abs().max() / Xt.abs().max())
            rec["speedup_vs_solve_ex"] = round(rec["torch_solve_ex_us"] / rec["ours_factor_plus_solve_us"], 2)
            rec["speedup_vs_torch_cholesky"] = round(rec["torch_cholesky_ex_plus_cholesky_solve_us"] / rec["ours_factor_plus_solve_us"], 2)
            rec["factor_GFLOPs"] = round(B * n ** 3 / 3 / rec["ours_factor_us"] / 1e3, 1)
            for name, fn in sides.items():
                rec[name.replace("_us", "_peak_extra_MiB")] = peak_extra(fn)
            emit_line(rec)
            del A, b, L, X, Xt

        # the assembly kernel beside its torch composition, on a CPD state of the workload's shape
        B, M, N = 32, 1024, 1024
        pairs = [cpd_oracle.sheet_pair(N=N, M=M, seed=s) for s in range(B)]
        Xc, Yc = torch.stack([p[0] for p in pairs]).to(dev), torch.stack([p[1] for p in pairs]).to(dev)
        reg = pcr.DeformableRegistration(Xc, Yc, alpha=co.ALPHA, beta=co.BETA, max_iterations=1, tolerance=0)
        reg.register()
        G, sigma2 = reg._G, reg._sigma2
        P1, _, PX, _ = reg._expectation()
        eye = torch.eye(M, dtype=torch.float64, device=dev)

        def composition():
            d = P1.sqrt()
            S = d[:, :, None] * G * d[:, None, :] + (co.ALPHA * sigma2)[:, None, None] * eye
            num = PX - P1[:, :, None] * Yc
            return S, torch.where(d[:, :, None] > 0, num / d[:, :, None], torch.zeros_like(num)), d

        sides = {"ours_us": lambda: F.cpd_spd_system(G, P1, PX, Yc, sigma2, co.ALPHA), "torch_composition_us": composition}
        rec = dict(kernel="cpd_spd_system", B=B, M=M, **alternating(sides, iters=9))
        rec["ours_peak_extra_MiB"], rec["torch_composition_peak_extra_MiB"] = peak_extra(sides["ours_us"]), peak_extra(composition)
        rec["speedup"] = round(rec["torch_composition_us"] / rec["ours_us"], 2)
        emit_line(rec)
        del reg, G, P1, PX, eye

    # the whole run: 100 iterations (tolerance 0), both solvers in one process, alternating
    def run(solver):
        reg = pcr.DeformableRegistration(Xc, Yc, alpha=co.ALPHA, beta=co.BETA, max_iterations=100, tolerance=0, solver=solver)
        return reg.register()[0]

    rounds = int(os.environ.get("FSG_CHOL_BENCH_ROUNDS", "2"))
    t = alternating({"cholesky_us": lambda: run('cholesky'), "lu_us": lambda: run('lu')}, iters=rounds, warm=0)
    rec = dict(kernel="cpd_deformable_100_iterations", B=B, M=M, N=N, rounds=rounds, **t)
    rec["speedup"] = round(t["lu_us"] / t["cholesky_us"], 2)
    rec["cholesky_peak_extra_MiB"], rec["lu_peak_extra_MiB"] = peak_extra(lambda: run('cholesky')), peak_extra(lambda: run('lu'))
    emit_line(rec)
