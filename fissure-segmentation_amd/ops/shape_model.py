"""Shape-model ops: DG-SSM decode, the CPD E-step, k-means, thin-plate splines, weighted sample elimination, the OPTICS ordering,
the batched fp64 Cholesky solver and CPD's symmetric positive definite M-step system."""
import torch

from .. import _lib
from .._launch import _amp_bwd, _amp_fwd, _f32c, _need_gpu, _p, launch
from .packed import fps


# ------------------------------------------------------------------ DG-SSM: shape-model decode + similarity transform
SSM_MAX_MODES = _lib.SSM_MAX_MODES


class _SSMDecodeAffine(torch.autograd.Function):
    """shape_model/ssm.py:74-83 + models/dg_ssm.py:133-135 (compose_transform, transform_points): one launch forward, two
    backward; the decoded shape is recomputed in the backward, mean and eigenvectors are frozen (ssm.py:33)"""

    @staticmethod
    @_amp_fwd
    def forward(ctx, w, mean, evec, v, s, tr):
        wc, mc, ec = _f32c(w), _f32c(mean), _f32c(evec)
        B, M = wc.shape
        P = mc.numel() // 3
        affine = v is not None
        vc, sc, tc = (_f32c(v), _f32c(s), _f32c(tr)) if affine else (None, None, None)
        out = torch.empty(B, P, 3, dtype=torch.float32, device=w.device)
        launch(w.device, "fsg_ssm_decode_fwd_f32", _p(wc), _p(mc), _p(ec), _p(vc), _p(sc), _p(tc), B, P, M, _p(out))
        ctx.save_for_backward(wc, mc, ec, vc, sc)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        wc, mc, ec, vc, sc = ctx.saved_tensors
        B, M = wc.shape
        P = mc.numel() // 3
        dev = wc.device
        dw = torch.empty_like(wc)
        dv, ds, dt = (torch.empty(B, 3, dtype=torch.float32, device=dev) for _ in range(3)) if vc is not None else (None,) * 3
        ws = _lib.workspace("fsg_ssm_decode_bwd", B, P, M, device=dev)
        launch(dev, "fsg_ssm_decode_bwd_f32", _p(_f32c(g)), _p(wc), _p(mc), _p(ec), _p(vc), _p(sc), B, P, M, _p(dw), _p(dv),
               _p(ds), _p(dt), _p(ws), ws.numel())
        return dw, None, None, dv, ds, dt


def ssm_decode_affine(w, mean, evec, v=None, s=None, tr=None):
    """w (B,M) mode weights, mean (3P) [or (1,3P)], evec (3P,M) [or (1,3P,M)] -> (B,P,3): the decoded shapes
    mean + evec w, moved -- when v, s, tr (B,3) are given -- by x -> (x R(v)) * s + tr with R = so3_exp_map(v) in the
    row-vector convention of augmentations.Transform3d.  Differentiable in w, v, s, tr; s may be (B,1)."""
    _need_gpu(w, mean, evec, v, s, tr)
    evec = evec.reshape(-1, evec.shape[-1])
    mean = mean.reshape(-1)
    if w.dim() != 2 or w.shape[1] != evec.shape[1] or mean.numel() != evec.shape[0] or mean.numel() % 3 != 0:
        raise ValueError(f"expected w (B,M), mean (3P), evec (3P,M), got {tuple(w.shape)}, {tuple(mean.shape)}, "
                         f"{tuple(evec.shape)}")
    if (v is None) != (s is None) or (v is None) != (tr is None):
        raise ValueError("v, s and tr come together (all or none)")
    if v is not None:
        B = w.shape[0]
        if tuple(v.shape) != (B, 3) or tuple(tr.shape) != (B, 3) or s.dim() != 2 or s.shape[0] != B or s.shape[1] not in (1, 3):
            raise ValueError(f"expected v, tr (B,3) and s (B,3) or (B,1), got {tuple(v.shape)}, {tuple(tr.shape)}, "
                             f"{tuple(s.shape)}")
        s = s.expand(B, 3)
    return _SSMDecodeAffine.apply(w, mean, evec, v, s, tr)


# ------------------------------------------------------------------ coherent point drift, E-step (shape_model/point_cloud_registration.py)
def cpd_estep(X, TY, sigma2, w=0.):
    """The reductions of CPD's responsibility matrix P (M, N) that the M-steps need, without P (fsg_cpd_estep_f32).

    X (B,N,3) fixed points or one (N,3) cloud shared by the batch, TY (B,M,3) transformed moving points, sigma2 (B) on the
    device (it is never read on the host), w in [0, 1) the outlier weight -> (P1 (B,M), Pt1 (B,N), PX (B,M,3), Np (B)), fp32.
    Deterministic, and item b's outputs do not depend on the other items.  An evaluation primitive, not differentiable."""
    _need_gpu(X, TY, sigma2)
    if TY.dim() != 3 or TY.shape[2] != 3 or X.dim() not in (2, 3) or X.shape[-1] != 3 or (X.dim() == 3 and X.shape[0] != TY.shape[0]):
        raise ValueError(f"expected X (B,N,3) or (N,3) and TY (B,M,3), got {tuple(X.shape)} and {tuple(TY.shape)}")
    B, M, _ = TY.shape
    N = X.shape[-2]
    if N < 1 or M < 1:
        raise ValueError(f"cpd_estep: empty cloud (N={N}, M={M})")
    if sigma2.numel() != B:
        raise ValueError(f"expected one sigma2 per item ({B}), got {tuple(sigma2.shape)}")
    if not 0. <= w < 1.:
        raise ValueError(f"the outlier weight w must lie in [0, 1), got {w}")
    with torch.no_grad():
        xc, yc, sc = _f32c(X), _f32c(TY), _f32c(sigma2).reshape(B)
        dev = yc.device
        P1 = torch.empty(B, M, dtype=torch.float32, device=dev)
        Pt1 = torch.empty(B, N, dtype=torch.float32, device=dev)
        PX = torch.empty(B, M, 3, dtype=torch.float32, device=dev)
        Np = torch.empty(B, dtype=torch.float32, device=dev)
        ws = _lib.workspace("fsg_cpd_estep", B, N, M, device=dev)
        launch(dev, "fsg_cpd_estep_f32", _p(xc), 3 * N if xc.dim() == 3 else 0, _p(yc), _p(sc), float(w), B, N, M, _p(P1),
               _p(Pt1), _p(PX), _p(Np), _p(ws), ws.numel())
    return P1, Pt1, PX, Np


# ------------------------------------------------------------------ k-means (shape_model/generate_corresponding_points.py:44-48)
KMEANS_CHECK_EVERY = 5   # iterations between two looks of the host at the "any item still active" word


def _kmeans_args(points, centroids, who):
    if points.dim() != 3 or points.shape[2] != 3 or centroids.dim() != 3 or centroids.shape[2] != 3 \
            or centroids.shape[0] != points.shape[0]:
        raise ValueError(f"{who}: expected points (B,n,3) and centroids (B,K,3), got {tuple(points.shape)} and "
                         f"{tuple(centroids.shape)}")
    B, n, _ = points.shape
    K = centroids.shape[1]
    if n < 1 or n > _lib.KMEANS_MAX_POINTS:
        raise ValueError(f"{who}: n={n} points per item, the kernel serves 1 <= n <= {_lib.KMEANS_MAX_POINTS}")
    if not 1 <= K <= min(n, _lib.KMEANS_MAX_K):
        raise ValueError(f"{who}: K={K} clusters, the kernel serves 1 <= K <= min(n, {_lib.KMEANS_MAX_K}) (n={n})")
    _need_gpu(points, centroids)
    if points.device != centroids.device:
        raise ValueError(f"{who}: points are on {points.device}, centroids on {centroids.device}")
    return B, n, K


class _KMeansRun:
    """the device state of one run: workspace (accumulators, scales, threshold, active flags), labels and the per-item outputs"""

    def __init__(self, points, centroids, tol, prev_labels=None):
        B, n, K = self.dims = points.shape[0], points.shape[1], centroids.shape[1]
        dev = self.dev = points.device
        self.points, self.centroids = points, centroids
        self.labels = torch.full((B, n), -1, dtype=torch.int32, device=dev) if prev_labels is None else prev_labels
        self.counts = torch.empty(B, K, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        self.info = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self.ws = _lib.workspace("fsg_kmeans", B, n, K, device=dev)
        launch(dev, "fsg_kmeans_prepare_f32", _p(points), _p(centroids), B, n, K, float(tol), _p(self.ws), self.ws.numel())

    def launch(self, entry):
        B, n, K = self.dims
        launch(self.dev, entry, _p(self.points), _p(self.centroids), _p(self.labels), B, n, K, _p(self.ws), self.ws.numel(),
               _p(self.counts), _p(self.stats), _p(self.info))


def kmeans_step(points, centroids, prev_labels=None):
    """One Lloyd iteration of B independent k-means problems (fsg_kmeans_step_f32): points (B,n,3), centroids (B,K,3),
    prev_labels (B,n) integer or None -> (labels (B,n) int32, new_centroids (B,K,3) fp32, counts (B,K) int32, inertia (B,) fp64,
    n_changed (B,) int32).

    labels[i] = argmin_k ((dx dx + dy dy) + dz dz) in fp32, the lowest k on ties; inertia is the sum of those squared distances,
    that is the inertia of `centroids`, not of new_centroids; n_changed counts labels that differ from prev_labels (all n
    without them); a cluster without points keeps its centroid (counts tells which).  Sums are int64 fixed-point: the same
    inputs give the same bits, whatever else is in the batch.  The inputs are not modified.  Not differentiable."""
    B, n, K = _kmeans_args(points, centroids, "kmeans_step")
    if B == 0:
        raise ValueError("kmeans_step: empty batch")
    if prev_labels is not None:
        _need_gpu(prev_labels)
        if tuple(prev_labels.shape) != (B, n) or prev_labels.is_floating_point():
            raise ValueError(f"kmeans_step: prev_labels must be integers of shape {(B, n)}, got {tuple(prev_labels.shape)} "
                             f"{prev_labels.dtype}")
    with torch.no_grad():
        prev = None if prev_labels is None else prev_labels.to(torch.int32, copy=True).contiguous()
        run = _KMeansRun(_f32c(points), _f32c(centroids).clone(), 0., prev)
        run.launch("fsg_kmeans_step_f32")
    return run.labels, run.centroids, run.counts, run.stats[:, 0].clone(), run.info[:, 0].clone()


def kmeans(points, n_clusters=None, init='fps', max_iter=300, tol=1e-4, start=0, return_info=False):
    """Lloyd's k-means of B independent 3-D clouds on the GPU: points (n,3) or (B,n,3) -> (centroids (B,K,3) fp32, labels (B,n)
    int64, inertia (B,) fp64, n_iter (B,) int32); a 2-D input comes back without the batch axis.

    `init` is 'fps' -- farthest point sampling (fsg_fps_f32) of n_clusters points of every item, started at row `start`; the
    selected rows are the first centres -- or a tensor (B,K,3) / (K,3) of explicit centres (then n_clusters may be omitted).
    There is no random seeding and no n_init: the run is deterministic, bit for bit, and an item's result does not depend on
    the batch it is in.  An item stops when no label changes or when the summed squared centre shift is at most
    tol * mean(var(points, axis=0)) (sklearn's rule) or after max_iter iterations, and is frozen from then on; the host looks at
    one "any item active" word every KMEANS_CHECK_EVERY iterations.  A cluster that loses all its points keeps its centre
    (scipy.cluster.vq.kmeans2's behaviour; sklearn relocates it).  The returned labels and inertia are those OF the returned
    centres (one last assign).  `return_info` appends a dict with `counts` (B,K) and `n_empty` (B,) of that assignment."""
    if not torch.is_tensor(points):
        raise TypeError(f"kmeans: points must be a torch tensor on the GPU, got {type(points).__name__}")
    squeeze = points.dim() == 2
    if squeeze:
        points = points[None]
    if points.dim() != 3 or points.shape[2] != 3 or not points.is_floating_point():
        raise ValueError(f"kmeans: expected floating-point points (n,3) or (B,n,3), got {tuple(points.shape)} {points.dtype}")
    B, n, _ = points.shape
    if B == 0:
        raise ValueError("kmeans: empty batch")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise ValueError(f"kmeans: max_iter must be a non-negative integer, got {max_iter!r}")
    if not tol >= 0:
        raise ValueError(f"kmeans: tol must not be negative, got {tol!r}")
    if torch.is_tensor(init):
        cen = init[None] if init.dim() == 2 else init
        if n_clusters is not None and cen.dim() == 3 and cen.shape[1] != n_clusters:
            raise ValueError(f"kmeans: init holds {cen.shape[1]} centres, n_clusters={n_clusters}")
        _kmeans_args(points, cen, "kmeans")
    elif isinstance(init, str) and init == 'fps':
        if n_clusters is None:
            raise ValueError("kmeans: init='fps' needs n_clusters")
        K = int(n_clusters)
        if not 1 <= K <= min(n, _lib.KMEANS_MAX_K):
            raise ValueError(f"kmeans: n_clusters={n_clusters}, the kernel serves 1 <= K <= min(n, {_lib.KMEANS_MAX_K}) (n={n})")
        if n > _lib.KMEANS_MAX_POINTS:
            raise ValueError(f"kmeans: n={n} points per item, the kernel serves n <= {_lib.KMEANS_MAX_POINTS}")
        if not 0 <= start < n:
            raise ValueError(f"kmeans: start={start} is no row of a cloud of {n} points")
        _need_gpu(points)
    else:
        raise ValueError(f"kmeans: init must be 'fps' or a tensor of centres, got {init!r}")
    with torch.no_grad():
        pc = _f32c(points)
        if torch.is_tensor(init):
            cen = _f32c(cen).clone()
        else:
            # the sampling kernel starts a segment at its first row: rotate every cloud so that row `start` is there
            rolled = torch.roll(pc, -start, 1).reshape(B * n, 3) if start else pc.reshape(B * n, 3)
            seg = torch.arange(1, B + 1, dtype=torch.int32, device=pc.device)
            rows = fps(rolled, seg * n, seg * K, B * K).long().view(B, K)    # rows of the packed, rotated clouds
            rows = (rows - (seg.long() - 1)[:, None] * n + start) % n
            cen = torch.gather(pc, 1, rows[:, :, None].expand(B, K, 3)).contiguous()
        run = _KMeansRun(pc, cen, tol)
        for it in range(max_iter):
            if it and it % KMEANS_CHECK_EVERY == 0 and not bool(run.info[:, 3].any()):   # the only synchronisation of the loop
                break
            run.launch("fsg_kmeans_step_f32")
        run.launch("fsg_kmeans_assign_f32")
        out = [run.centroids, run.labels.long(), run.stats[:, 0].clone(), run.info[:, 2].clone()]
        extra = {"counts": run.counts, "n_empty": run.info[:, 1].clone()}
    if squeeze:
        out = [t[0] for t in out]
        extra = {k: v[0] for k, v in extra.items()}
    return (*out, extra) if return_info else tuple(out)


# ------------------------------------------------------------------ thin-plate splines (shape_model/point_cloud_registration.py:24-89,119-133)
TPS_MAX_CHANNELS = _lib.TPS_MAX_CHANNELS


def _tps_points(t, name, who):
    """(n,3) or (B,n,3) floating-point -> (B,n,3), and whether the batch axis was added"""
    if not torch.is_tensor(t) or t.dim() not in (2, 3) or t.shape[-1] != 3 or t.shape[-2] < 1 or not t.is_floating_point():
        got = f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{who}: {name} must be a floating-point (points, 3) or (batch, points, 3) tensor, got {got}")
    return (t[None], True) if t.dim() == 2 else (t, False)


def _tps_theta(theta, B, n, who):
    if not torch.is_tensor(theta) or theta.dtype != torch.float64:
        raise ValueError(f"{who}: theta must be an fp64 tensor (tps_fit returns one), got "
                         f"{theta.dtype if torch.is_tensor(theta) else type(theta).__name__}")
    if theta.dim() == 2:
        theta = theta[None]
    if theta.dim() != 3 or theta.shape[0] != B or theta.shape[1] != n + 4:
        raise ValueError(f"{who}: theta must be ({B}, {n + 4}, C) for {B} x {n} control points, got {tuple(theta.shape)}")
    if not 1 <= theta.shape[2] <= TPS_MAX_CHANNELS:
        raise ValueError(f"{who}: C={theta.shape[2]} channels, the kernel serves 1 <= C <= {TPS_MAX_CHANNELS}")
    return theta


def _tps_same_device(who, *tensors):
    if len({t.device for t in tensors}) != 1:
        raise ValueError(f"{who}: the tensors are on different devices ({', '.join(str(t.device) for t in tensors)})")


def _tps_size(size, what):
    try:
        size = tuple(int(s) for s in size)
    except (TypeError, ValueError):
        size = ()
    if len(size) != 3 or min(size) < 1 or max(size) > 1 << 24 or size[0] * size[1] * size[2] >= 1 << 31:
        raise ValueError(f"{what} must be three positive integers (D, H, W) with fewer than 2^31 nodes, got {size!r}")
    return size


def tps_system(control, lambd=0.):
    """The matrix of the reference's TPS.fit (fsg_tps_system_f64): control (B,n,3) or (n,3) -> (B,n+4,n+4) or (n+4,n+4) fp64,
    u(|c_i - c_j|) + lambd I with u(r) = r^2 log(r + 1e-6), bordered by [1 | c], its transpose and zeros.  Distances are sums of
    squared differences in fp64 (ours, not the reference's fp32 ra + rb - 2 ab): symmetric bit for bit, the diagonal exactly
    lambd."""
    c, squeeze = _tps_points(control, "control", "tps_system")
    _need_gpu(c)
    B, n, _ = c.shape
    if n > 32764:
        raise ValueError(f"tps_system: n={n} control points, the kernel serves n <= 32764")
    with torch.no_grad():
        cc = _f32c(c)
        A = torch.empty(B, n + 4, n + 4, dtype=torch.float64, device=cc.device)
        launch(cc.device, "fsg_tps_system_f64", _p(cc), B, n, float(lambd), _p(A))
    return A[0] if squeeze else A


TPS_SOLVERS = ('lu', 'nullspace')


def _tps_values(control, values, squeeze, who):
    """values (B,n,C), or (n,C) beside a control (n,3) -> (B,n,C)"""
    if not torch.is_tensor(values) or not values.is_floating_point() or values.dim() != control.dim() \
            or values.shape[:-1] != control.shape[:-1]:
        got = f"{tuple(values.shape)} {values.dtype}" if torch.is_tensor(values) else type(values).__name__
        raise ValueError(f"{who}: values must be floating-point {tuple(control.shape[:-1])} + (C,), got {got}")
    v = values[None] if squeeze else values
    if not 1 <= v.shape[2] <= TPS_MAX_CHANNELS:
        raise ValueError(f"{who}: C={v.shape[2]} channels, the kernels serve 1 <= C <= {TPS_MAX_CHANNELS}")
    return v


def _tps_lu(c, v, lambd):
    """theta (B,n+4,C) of the saddle systems by torch's batched fp64 linalg.solve"""
    n = c.shape[1]
    A = tps_system(c, lambd)
    rhs = torch.zeros(A.shape[0], n + 4, v.shape[2], dtype=torch.float64, device=c.device)
    rhs[:, :n] = v
    return torch.linalg.solve(A, rhs)


def tps_fit(control, values, lambd=0., fit_batch=32, solver='lu'):
    """TPS.fit for a batch: control (B,n,3), values (B,n,C) (or (n,3), (n,C)) -> theta (B,n+4,C) fp64, the n spline weights and
    the four affine rows, `fit_batch` systems at a time (100 systems of 1028^2 in fp64 are 0.85 GB).  n >= 4 points not in one
    plane (or lambd > 0 with distinct points) make the system regular.
    solver='lu': the systems come from `tps_system`, the solve is torch's batched fp64 linalg.solve; a singular one raises as
    linalg.solve does.
    solver='nullspace': `tps_nullspace_fit`, whose status is read once per chunk.  Items whose points lie in one plane (status
    < 0) raise a RuntimeError that names them; items whose reduced system is not positive definite (status > 0: a negative
    lambd, or lambd = 0 with near-coincident points, which can be regular without being definite) are solved again through
    the 'lu' route, one at a time, and only those."""
    if solver not in TPS_SOLVERS:
        raise ValueError(f"tps_fit: solver must be one of {TPS_SOLVERS}, got {solver!r}")
    c, squeeze = _tps_points(control, "control", "tps_fit")
    v = _tps_values(control, values, squeeze, "tps_fit")
    if isinstance(fit_batch, bool) or not isinstance(fit_batch, int) or fit_batch < 1:
        raise ValueError(f"tps_fit: fit_batch must be a positive integer, got {fit_batch!r}")
    _need_gpu(c, v)
    _tps_same_device("tps_fit", c, v)
    B, n, C = v.shape
    with torch.no_grad():
        theta = torch.empty(B, n + 4, C, dtype=torch.float64, device=c.device)
        for b0 in range(0, B, fit_batch):
            cb, vb = c[b0:b0 + fit_batch], v[b0:b0 + fit_batch]
            if solver == 'lu':
                theta[b0:b0 + fit_batch] = _tps_lu(cb, vb, lambd)
                continue
            theta[b0:b0 + fit_batch], info = tps_nullspace_fit(cb, vb, lambd)
            info = info.tolist()   # the one host read of the chunk
            flat = [b0 + i for i, s in enumerate(info) if s < 0]
            if flat:
                raise RuntimeError(f"tps_fit: the control points of item(s) {flat} do not span three dimensions (fewer than 4 "
                                   f"points, points in one plane, or a NaN): the spline's system is singular")
            for i, s in enumerate(info):
                if s > 0:
                    theta[b0 + i] = _tps_lu(cb[i:i + 1], vb[i:i + 1], lambd)[0]
    return theta[0] if squeeze else theta


def tps_nullspace_system(control, lambd=0.):
    """Steps 1-4 of the null-space route (fsg_tps_ns_system_f64): control (B,n,3) or (n,3) -> (V, tau, R, S, info).  With
    P = [1 | c] = Q [R; 0]: V (B,n,4) the Householder vectors (LAPACK dgeqr2's convention), tau (B,4), R (B,4,4) upper
    triangular, S (B,n-4,n-4) = (Q^T (K + lambd I) Q)[4:, 4:] with K as `tps_system` writes it -- LOWER triangle only, the rest
    is uninitialised; (B,0,0) for n <= 4 -- and info (B) int32 on the device: 0, or -k for the first |R_kk| <= n 2^-52 max |R_jj|
    (points in one plane, fewer than 4 points, a NaN).  K is never stored.  fp64; not differentiable."""
    c, squeeze = _tps_points(control, "control", "tps_nullspace_system")
    _need_gpu(c)
    B, n, _ = c.shape
    m = max(n - 4, 0)
    if m > CHOL_MAX_N or B > CHOL_MAX_BATCH:
        raise ValueError(f"tps_nullspace_system: {B} x {n} control points, the kernels serve n - 4 <= {CHOL_MAX_N} and at most "
                         f"{CHOL_MAX_BATCH} items")
    with torch.no_grad():
        cc = _f32c(c)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=cc.device)   # noqa: E731
        V, tau, R, S = new(B, n, 4), new(B, 4), new(B, 4, 4), new(B, m, m)
        work = new(B * n * _lib.TPS_NS_SYSTEM_WORK_PER_POINT)
        info = torch.empty(B, dtype=torch.int32, device=cc.device)
        launch(cc.device, "fsg_tps_ns_system_f64", _p(cc), B, n, float(lambd), _p(V), _p(tau), _p(R), _p(S) if m else None,
               _p(info), _p(work))
    out = (V, tau, R, S, info)
    return tuple(t[0] for t in out) if squeeze else out


def tps_nullspace_fit(control, values, lambd=0.):
    """TPS.fit by the null-space route: control (B,n,3), values (B,n,C) (or (n,3), (n,C)) -> (theta (B,n+4,C) fp64, info).
    `tps_nullspace_system`, `cholesky_factor` of S in place, then fsg_tps_ns_solve_f64 around `cholesky_solve`.  Nothing is read
    on the host, so the call can be captured in a graph: info (B) int32 stays on the device -- 0, -k (the rank status above) or
    j (the reduced system's leading minor of order j is not positive) -- and the theta of an item whose info is not 0 is
    unspecified.  For n = 4 the reduced system is empty and no factorisation is launched.  Not differentiable."""
    c, squeeze = _tps_points(control, "control", "tps_nullspace_fit")
    v = _tps_values(control, values, squeeze, "tps_nullspace_fit")
    _need_gpu(c, v)
    _tps_same_device("tps_nullspace_fit", c, v)
    B, n, C = v.shape
    with torch.no_grad():
        cc = _f32c(c)
        vc = v.detach().to(torch.float64).contiguous()
        V, tau, R, S, info = tps_nullspace_system(cc, lambd)
        if n > 4:
            L, chol = cholesky_factor(S, overwrite=True)
            info = torch.where(info != 0, info, chol)
        theta = torch.empty(B, n + 4, C, dtype=torch.float64, device=cc.device)
        work = torch.empty(B * n * C * _lib.TPS_NS_SOLVE_WORK_PER_VALUE, dtype=torch.float64, device=cc.device)
        launch(cc.device, "fsg_tps_ns_solve_f64", _p(cc), _p(vc), _p(V), _p(tau), _p(R), _p(L) if n > 4 else None, B, n, C,
               float(lambd), _p(work), _p(theta))
    return (theta[0], info[0]) if squeeze else (theta, info)


def tps_eval(queries, control, theta):
    """TPS.z (fsg_tps_eval_f32): the spline theta (B,n+4,C) fp64 on control (B,n,3) at queries (B,Q,3) -> (B,Q,C) fp32.
    `queries` may instead be a lattice size (D1,H1,W1): the nodes of an align_corners=True lattice over [-1,1]^3 in
    (z,y,x)-major order with (x,y,z) coordinates, as thin_plate_dense builds them with affine_grid -- no coordinate tensor is
    read; -> (B, D1 H1 W1, C).  u and the sum over the control points are fp64.  2-D inputs are a batch of one."""
    c, squeeze = _tps_points(control, "control", "tps_eval")
    B, n, _ = c.shape
    th = _tps_theta(theta, B, n, "tps_eval")
    C = th.shape[2]
    if torch.is_tensor(queries):
        q, _ = _tps_points(queries, "queries", "tps_eval")
        if q.shape[0] != B or queries.dim() != control.dim():
            raise ValueError(f"tps_eval: queries {tuple(queries.shape)} and control {tuple(control.shape)} do not share a batch")
        _need_gpu(q, c, th)
        _tps_same_device("tps_eval", q, c, th)
        Q, lattice = q.shape[1], (0, 0, 0)
    else:
        lattice = _tps_size(queries, "tps_eval: a lattice")
        q, Q = None, lattice[0] * lattice[1] * lattice[2]
        _need_gpu(c, th)
        _tps_same_device("tps_eval", c, th)
    with torch.no_grad():
        cc, tc = _f32c(c), th.detach().contiguous()
        qc = _f32c(q) if q is not None else None
        out = torch.empty(B, Q, C, dtype=torch.float32, device=cc.device)
        launch(cc.device, "fsg_tps_eval_f32", _p(qc), _p(cc), _p(tc), B, Q, n, C, *lattice, _p(out))
    return out[0] if squeeze else out


def tps_grid_sample(grid, control, theta, size, step=4):
    """What the reference reads out of its dense displacement field, without the field (fsg_tps_grid_sample_f32):
    F.grid_sample(align_corners=False, zeros padding) at grid (B,Q,3) (x,y,z in [-1,1], x along the last axis) of the trilinear
    align_corners=True upsample to size = (D,H,W) of the spline theta (B,n+4,C) on control (B,n,3), evaluated on the lattice
    (D//step, H//step, W//step) -> (B,Q,C) fp32.  A sample depends on at most 3 coarse nodes per axis; the spline is evaluated
    at those only.  A sample whose taps all lie outside the volume is exactly 0.  2-D inputs are a batch of one."""
    c, squeeze = _tps_points(control, "control", "tps_grid_sample")
    B, n, _ = c.shape
    th = _tps_theta(theta, B, n, "tps_grid_sample")
    g, _ = _tps_points(grid, "grid", "tps_grid_sample")
    if g.shape[0] != B or grid.dim() != control.dim():
        raise ValueError(f"tps_grid_sample: grid {tuple(grid.shape)} and control {tuple(control.shape)} do not share a batch")
    size = _tps_size(size, "tps_grid_sample: size")
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"tps_grid_sample: step must be a positive integer, got {step!r}")
    if min(size) < step:
        raise ValueError(f"tps_grid_sample: every axis of size {size} must hold at least step={step} voxels (the coarse lattice "
                         f"would be empty)")
    coarse = tuple(s // step for s in size)
    _need_gpu(g, c, th)
    _tps_same_device("tps_grid_sample", g, c, th)
    Q, C = g.shape[1], th.shape[2]
    with torch.no_grad():
        gc, cc, tc = _f32c(g), _f32c(c), th.detach().contiguous()
        out = torch.empty(B, Q, C, dtype=torch.float32, device=cc.device)
        launch(cc.device, "fsg_tps_grid_sample_f32", _p(gc), _p(cc), _p(tc), B, Q, n, C, *size, *coarse, _p(out))
    return out[0] if squeeze else out


# ------------------------------------------------------------------ weighted sample elimination (open3d's sample_points_poisson_disk)
def _per_item_radius(v, B, dev, name):
    """a scalar or a (B,) tensor / sequence -> (B,) fp32 on `dev`"""
    if torch.is_tensor(v):
        _need_gpu(v)
        if v.numel() not in (1, B) or v.dim() > 1 or not v.is_floating_point():
            raise ValueError(f"sample_elimination: {name} must be a scalar or a floating-point ({B},) tensor, got "
                             f"{tuple(v.shape)} {v.dtype}")
        return v.detach().to(device=dev, dtype=torch.float32).reshape(-1).expand(B)
    t = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    if t.numel() not in (1, B):
        raise ValueError(f"sample_elimination: {name} must be a scalar or hold one value per item ({B}), got {t.numel()}")
    return t.to(torch.float32).to(dev).expand(B)


def sample_elimination(points, n_keep, r_max, r_min, return_order=False):
    """Weighted sample elimination (Yuksel 2015) of B independent 3-D clouds on the GPU (fsg_sample_elimination_f32): points
    (M,3) or (B,M,3) -> keep (B,n_keep) int64, the surviving rows in ascending order [, order (B, M - n_keep) int64, the rows in
    the order they were removed]; a 2-D input comes back without the batch axis.

    r_max (the paper's 2 r_max: samples closer than it are neighbours) and r_min are scalars or (B,); tensors stay on the
    device (a Python number is copied there: inside a graph capture pass device tensors).  Pair weight, in fp32:
    d = max(|p_i - p_j|, r_min), w = max(1 - d / r_max, 0)^8, quantised to rint(w 2^24); a
    sample's weight is the integer sum over its alive neighbours; every round removes the heaviest alive sample, the lowest row
    on ties, and lowers its neighbours' weights.  r_max <= 0, or nobody within r_max of anybody: rows leave in index order.
    Deterministic bit for bit, and an item's result does not depend on the batch it is in.  No host synchronisation.  Not
    differentiable."""
    if not torch.is_tensor(points):
        raise TypeError(f"sample_elimination: points must be a torch tensor on the GPU, got {type(points).__name__}")
    squeeze = points.dim() == 2
    if squeeze:
        points = points[None]
    if points.dim() != 3 or points.shape[2] != 3 or not points.is_floating_point():
        raise ValueError(f"sample_elimination: expected floating-point points (M,3) or (B,M,3), got {tuple(points.shape)} "
                         f"{points.dtype}")
    B, M, _ = points.shape
    if B == 0:
        raise ValueError("sample_elimination: empty batch")
    if B > 65535:
        raise ValueError(f"sample_elimination: B={B} items, the kernel serves B <= 65535")
    if not 1 <= M <= _lib.SAMPLE_ELIMINATION_MAX_POINTS:
        raise ValueError(f"sample_elimination: M={M} points per item, the kernel serves 1 <= M <= "
                         f"{_lib.SAMPLE_ELIMINATION_MAX_POINTS}")
    if isinstance(n_keep, bool) or not isinstance(n_keep, int) or not 1 <= n_keep <= M:
        raise ValueError(f"sample_elimination: n_keep must be an integer with 1 <= n_keep <= M={M}, got {n_keep!r}")
    _need_gpu(points)
    dev = points.device
    with torch.no_grad():
        radii = torch.stack([_per_item_radius(r_max, B, dev, "r_max"), _per_item_radius(r_min, B, dev, "r_min")], 1).contiguous()
        pc = _f32c(points)
        keep = torch.empty(B, n_keep, dtype=torch.int32, device=dev)
        order = torch.empty(B, M - n_keep, dtype=torch.int32, device=dev) if return_order else None
        ws = _lib.workspace("fsg_sample_elimination", B, M, device=dev)
        launch(dev, "fsg_sample_elimination_f32", _p(pc), _p(radii), B, M, n_keep, _p(keep), _p(order), _p(ws), ws.numel())
        out = [keep.long()] + ([order.long()] if return_order else [])
    if squeeze:
        out = [t[0] for t in out]
    return tuple(out) if return_order else out[0]


# ------------------------------------------------------------------ OPTICS (shape_model/generate_corresponding_points.py:50-62)
def optics(points, min_samples, max_eps=float("inf"), return_squared=False):
    """OPTICS reachability graph of B independent 3-D clouds on the GPU (fsg_optics_f32): points (n,3) or (B,n,3) -> (ordering
    (B,n) int64, core_distances (B,n) fp64, reachability (B,n) fp64, predecessor (B,n) int64); a 2-D input comes back without
    the batch axis.  ordering lists the points in the order they were processed; the other three are indexed by point
    (reachability inf and predecessor -1 where a walk starts, core distance inf with fewer than min_samples points within
    max_eps), as the attributes of sklearn.cluster.OPTICS are.

    max_eps is a number (> 0, may be inf) or a (B,) tensor with one radius per item; a tensor stays on the device and its
    values are not checked there.  Distances are Euclidean, computed in fp64 from the fp32 coordinates and compared as squares;
    with return_squared the squares come back as the kernel wrote them, otherwise their `torch.sqrt`.  A point's core distance
    is the distance to its min_samples-th nearest point, itself counted; the next point is the unprocessed one with the
    smallest reachability, the lowest row on ties (also among the inf ones).  sklearn's rounding of the distances to 15 decimals
    is not applied.  Deterministic bit for bit (the squares, ordering and predecessor), and an item's result does not depend on
    the batch it is in.  No host synchronisation.  Not differentiable."""
    if not torch.is_tensor(points):
        raise TypeError(f"optics: points must be a torch tensor on the GPU, got {type(points).__name__}")
    squeeze = points.dim() == 2
    if squeeze:
        points = points[None]
    if points.dim() != 3 or points.shape[2] != 3 or not points.is_floating_point():
        raise ValueError(f"optics: expected floating-point points (n,3) or (B,n,3), got {tuple(points.shape)} {points.dtype}")
    B, n, _ = points.shape
    if B == 0:
        raise ValueError("optics: empty batch")
    if B > 65535:
        raise ValueError(f"optics: B={B} items, the kernel serves B <= 65535")
    if n > _lib.OPTICS_MAX_POINTS:
        raise ValueError(f"optics: n={n} points per item, the kernel serves n <= {_lib.OPTICS_MAX_POINTS}")
    if isinstance(min_samples, bool) or not isinstance(min_samples, int) \
            or not 2 <= min_samples <= min(n, _lib.OPTICS_MAX_MIN_SAMPLES):
        raise ValueError(f"optics: min_samples must be an integer with 2 <= min_samples <= min(n, "
                         f"{_lib.OPTICS_MAX_MIN_SAMPLES}) (n={n}), got {min_samples!r}")
    if torch.is_tensor(max_eps):
        if max_eps.dim() != 1 or max_eps.shape[0] != B or not max_eps.is_floating_point():
            raise ValueError(f"optics: max_eps must be a number or a floating-point ({B},) tensor, got {tuple(max_eps.shape)} "
                             f"{max_eps.dtype}")
        _need_gpu(points, max_eps)
        if max_eps.device != points.device:
            raise ValueError(f"optics: points are on {points.device}, max_eps on {max_eps.device}")
        eps = max_eps.detach().to(torch.float64).contiguous()
    else:
        if isinstance(max_eps, bool) or not isinstance(max_eps, (int, float)) or not max_eps > 0:
            raise ValueError(f"optics: max_eps must be a positive number (inf allowed) or a ({B},) tensor, got {max_eps!r}")
        _need_gpu(points)
        eps = torch.full((B,), float(max_eps), dtype=torch.float64, device=points.device)
    dev = points.device
    with torch.no_grad():
        pc = _f32c(points)
        ordering = torch.empty(B, n, dtype=torch.int32, device=dev)
        pred = torch.empty(B, n, dtype=torch.int32, device=dev)
        core2 = torch.empty(B, n, dtype=torch.float64, device=dev)
        reach2 = torch.empty(B, n, dtype=torch.float64, device=dev)
        ws = _lib.workspace("fsg_optics", B, n, min_samples, device=dev)
        launch(dev, "fsg_optics_f32", _p(pc), _p(eps), B, n, min_samples, _p(ordering), _p(core2), _p(reach2), _p(pred), _p(ws),
               ws.numel())
        out = [ordering.long(), core2 if return_squared else torch.sqrt(core2), reach2 if return_squared else torch.sqrt(reach2),
               pred.long()]
    if squeeze:
        out = [t[0] for t in out]
    return tuple(out)


# ------------------------------------------------------------------ batched fp64 Cholesky (csrc/cholesky.hip) and CPD's SPD system
CHOL_BLOCK = _lib.CHOL_BLOCK
CHOL_MAX_N = _lib.CHOL_MAX_N
CHOL_MAX_BATCH = _lib.CHOL_MAX_BATCH
CHOL_MAX_RHS = _lib.CHOL_MAX_RHS


def _chol_matrix(A, name, who):
    """(n,n) or (B,n,n) fp64 -> (B,n,n), and whether the batch axis was added"""
    if not torch.is_tensor(A) or A.dtype != torch.float64 or A.dim() not in (2, 3) or A.shape[-1] != A.shape[-2]:
        got = f"{tuple(A.shape)} {A.dtype}" if torch.is_tensor(A) else type(A).__name__
        raise ValueError(f"{who}: {name} must be an fp64 (n, n) or (batch, n, n) tensor, got {got}")
    squeeze = A.dim() == 2
    A = A[None] if squeeze else A
    if not 1 <= A.shape[1] <= CHOL_MAX_N or A.shape[0] > CHOL_MAX_BATCH:
        raise ValueError(f"{who}: {name} is {tuple(A.shape)}, the kernels serve 1 <= n <= {CHOL_MAX_N} and at most {CHOL_MAX_BATCH} items")
    return A, squeeze


def _chol_rhs(rhs, B, n, squeeze, who):
    """(B,n,r) or (B,n) fp64 (without the batch axis when the matrix came without) -> (B,n,r), and whether r was added"""
    if not torch.is_tensor(rhs) or rhs.dtype != torch.float64:
        raise ValueError(f"{who}: the right-hand sides must be an fp64 tensor, got "
                         f"{rhs.dtype if torch.is_tensor(rhs) else type(rhs).__name__}")
    r = rhs[None] if squeeze else rhs
    vector = r.dim() == 2
    r = r[:, :, None] if vector else r
    if r.dim() != 3 or r.shape[0] != B or r.shape[1] != n:
        raise ValueError(f"{who}: right-hand sides {tuple(rhs.shape)} do not fit {B} systems of order {n}")
    if not 1 <= r.shape[2] <= CHOL_MAX_RHS:
        raise ValueError(f"{who}: r={r.shape[2]} right-hand sides, the kernel serves 1 <= r <= {CHOL_MAX_RHS}")
    return r, vector


def _chol_out(src, out, what, who):
    """a contiguous tensor holding `src`: `out` itself (checked, filled unless it is `src`) or a fresh copy"""
    if out is None:
        return src.clone(memory_format=torch.contiguous_format)
    if not torch.is_tensor(out) or out.shape != src.shape or out.dtype != src.dtype or out.device != src.device \
            or not out.is_contiguous():
        raise ValueError(f"{who}: `out` must be a contiguous {tuple(src.shape)} fp64 tensor on the device of {what}")
    if out.data_ptr() != src.data_ptr():
        out.copy_(src)
    return out


def cholesky_factor(A, out=None, overwrite=False):
    """A (B,n,n) or (n,n) fp64, symmetric positive definite -> (L, info): A = L L^T, L in the lower triangle (fsg_cholesky_f64).
    Only the lower triangle of A is read; the strict upper triangle of L holds whatever it held in A (torch.linalg.cholesky
    zeroes it).  info (B) int32 stays on the device: 0, or j when the leading minor of order j is not positive (a NaN pivot
    counts); L of such an item is unspecified from column j on.  A is left alone unless `overwrite=True` (A must then be
    contiguous) or `out=` names the tensor to factor in.  An evaluation primitive, not differentiable."""
    A3, squeeze = _chol_matrix(A, "A", "cholesky_factor")
    _need_gpu(A3)
    with torch.no_grad():
        if overwrite:
            if out is not None or not A3.is_contiguous():
                raise ValueError("cholesky_factor: overwrite=True factors A in place: A must be contiguous, and `out` makes no sense")
            L = A3.detach()
        else:
            L = _chol_out(A3.detach(), out[None] if (squeeze and torch.is_tensor(out) and out.dim() == 2) else out, "A",
                          "cholesky_factor")
        B, n, _ = L.shape
        info = torch.empty(B, dtype=torch.int32, device=L.device)
        launch(L.device, "fsg_cholesky_f64", _p(L), B, n, _p(info))
    return (L[0] if squeeze else L), info


def cholesky_solve(L, rhs, out=None, overwrite=False):
    """L (B,n,n) or (n,n) from `cholesky_factor`, rhs (B,n,r) or (B,n) fp64 with r <= CHOL_MAX_RHS -> X of the shape of rhs with
    L L^T X = rhs (fsg_cholesky_solve_f64).  The strict upper triangle of L is not read.  rhs is left alone unless
    `overwrite=True` (contiguous rhs, solved in place) or `out=`.  Not differentiable."""
    L3, squeeze = _chol_matrix(L, "L", "cholesky_solve")
    B, n, _ = L3.shape
    r3, vector = _chol_rhs(rhs, B, n, squeeze, "cholesky_solve")
    _need_gpu(L3, r3)
    if L3.device != r3.device:
        raise ValueError(f"cholesky_solve: L is on {L3.device}, the right-hand sides on {r3.device}")
    with torch.no_grad():
        if overwrite:
            if out is not None or not r3.is_contiguous():
                raise ValueError("cholesky_solve: overwrite=True solves in place: rhs must be contiguous, and `out` makes no sense")
            X = r3.detach()
        else:
            X = _chol_out(r3.detach(), out.reshape(r3.shape) if (torch.is_tensor(out) and out.is_contiguous()
                                                                  and out.numel() == r3.numel()) else out, "rhs", "cholesky_solve")
        launch(X.device, "fsg_cholesky_solve_f64", _p(L3.detach().contiguous()), _p(X), B, n, X.shape[2])
    X = X[:, :, 0] if vector else X
    return X[0] if squeeze else X


def spd_solve(A, rhs, overwrite=False):
    """-> (X, info) with A X = rhs for symmetric positive definite A (B,n,n) fp64: `cholesky_factor`, then `cholesky_solve`.
    X of an item whose info is not 0 is unspecified.  `overwrite=True` lets both calls work in place (A becomes L, rhs X)."""
    L, info = cholesky_factor(A, overwrite=overwrite)
    return cholesky_solve(L, rhs, overwrite=overwrite), info


def cpd_spd_system(G, P1, PX, Y, sigma2, alpha):
    """The M-step system of deformable CPD in its symmetric positive definite form (fsg_cpd_spd_system_f64), one pass:
    G (B,M,M), P1 (B,M), PX (B,M,3), Y (B,M,3), sigma2 (B) on the device, all fp64, and the number alpha -> (S, rhs, d) with
    d = sqrt(P1), S = diag(d) G diag(d) + alpha sigma2 I (LOWER triangle only; the rest of S is uninitialised) and
    rhs = (PX - P1 Y) / d, 0 where d = 0.  With S V = rhs, W = d V solves (diag(P1) G + alpha sigma2 I) W = PX - P1 Y.  A row
    with P1 = 0 gets exactly alpha sigma2 on the diagonal and a zero right-hand side, so its W is 0, as in the unsymmetric
    system.  Not differentiable."""
    ts = (G, P1, PX, Y, sigma2)
    if not all(torch.is_tensor(t) and t.dtype == torch.float64 for t in ts):
        raise ValueError("cpd_spd_system: G, P1, PX, Y and sigma2 must be fp64 tensors")
    if G.dim() != 3 or G.shape[1] != G.shape[2]:
        raise ValueError(f"cpd_spd_system: G must be (B, M, M), got {tuple(G.shape)}")
    B, M, _ = G.shape
    if tuple(P1.shape) != (B, M) or tuple(PX.shape) != (B, M, 3) or tuple(Y.shape) != (B, M, 3) or sigma2.numel() != B:
        raise ValueError(f"cpd_spd_system: expected P1 ({B},{M}), PX and Y ({B},{M},3) and one sigma2 per item, got "
                         f"{tuple(P1.shape)}, {tuple(PX.shape)}, {tuple(Y.shape)}, {tuple(sigma2.shape)}")
    if not 1 <= M <= CHOL_MAX_N or B > CHOL_MAX_BATCH:
        raise ValueError(f"cpd_spd_system: the kernel serves 1 <= M <= {CHOL_MAX_N} and at most {CHOL_MAX_BATCH} items")
    _need_gpu(*ts)
    if len({t.device for t in ts}) != 1:
        raise ValueError("cpd_spd_system: the tensors are on different devices")
    with torch.no_grad():
        Gc, p1, px, yc, s2 = (t.detach().contiguous() for t in ts)
        S = torch.empty(B, M, M, dtype=torch.float64, device=G.device)
        rhs = torch.empty(B, M, 3, dtype=torch.float64, device=G.device)
        d = torch.empty(B, M, dtype=torch.float64, device=G.device)
        launch(G.device, "fsg_cpd_spd_system_f64", _p(Gc), _p(p1), _p(px), _p(yc), _p(s2.reshape(B)), float(alpha), B, M, _p(S),
               _p(rhs), _p(d))
    return S, rhs, d
