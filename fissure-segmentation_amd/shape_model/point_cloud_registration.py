"""Coherent point drift (Myronenko & Song, "Point Set Registration: Coherent Point Drift", TPAMI 2010) for the
corresponding-point shapes that `SSM.fit` consumes -- the registration part of the reference's
shape_model/point_cloud_registration.py, which calls pycpd on the CPU for one case and one object at a time (:101-116 the
deformable step with alpha = 0.01 and beta = 10, :231-237 the joint rigid pre-registration, :136-177 the inverse transformation
sampled at the fixed points).

Here a registration object takes a whole batch: X (N,3) or (B,N,3) fixed, Y (M,3) or (B,M,3) moving.  The E-step -- the dense
(M, N) responsibilities and their three reductions -- is one fused HIP entry point, fp32 in and out (functional.cpd_estep), that never
stores the matrix; the M-step's 3 x 3 SVDs are torch.linalg in fp64, and so is the deformable M x M solve by default (the
system's condition number grows like M / (alpha sigma^2)).  `solver='cholesky'` takes the deformable solve to this package's own
kernels instead: A = diag(P1) G + alpha sigma^2 I is similar to the symmetric positive definite S = D G D + alpha sigma^2 I,
D = diag(sqrt(P1)); one kernel writes S, the scaled right-hand side and D (functional.cpd_spd_system), a blocked fp64 Cholesky on
the matrix pipe factors and solves it (functional.spd_solve), and W = D V.  A row with P1 = 0 decouples (W = 0 there, as in A).
Same mathematics, other rounding: the two solvers end a run about 1e-10 units apart in fp64 arithmetic.  sigma^2, the per-item `active` flag and the iteration counts stay on the device: an item that has met
its stopping rule is frozen, and the host looks at one "any active" word every `CHECK_EVERY` iterations.

Defaults and stopping rules are pycpd's: sigma^2 starts at sum |x - y|^2 / (3 N M); the rigid run stops when the objective q
changes by at most `tolerance`, the deformable run when sigma^2 does; a non-positive sigma^2 becomes tolerance / 10.

NOT reproduced: pycpd clamps tiny E-step denominators to machine epsilon, differently from version to version -- one version
thereby silently drops a fixed point that lies farther than about 8.5 sigma from every moving point.  The kernel evaluates the
exponent relative to each fixed point's nearest moving point and so keeps the mathematical value.  pycpd is not a dependency
of this package, and parity with it is unpinned: the yardstick is the fp64 restatement in tests/cpd_oracle.py.

numpy arrays go in the way the reference passes them and come out as numpy (the work still runs on the current GPU); torch
tensors must be on a GPU and stay there.  A 2-D Y is a batch of one, returned without the batch axis.

The thin-plate-spline interpolation (:24-89 `TPS` and `thin_plate_dense`, :119-133 `interpolate_displacements_tps`) is here too.
The reference fits a spline on the moved cloud, evaluates it on a lattice of a quarter of the image's resolution, upsamples that
to a dense displacement field of the whole image and reads the sample points out of it with grid_sample.  Here the system matrix
is one kernel (fp64, functional.tps_system), the solve torch's batched fp64 linalg.solve -- or, with solver='nullspace', this
package's own: the polynomial block is eliminated by a Householder QR and the rest is a Cholesky factorisation
(functional.tps_nullspace_fit) --, and the samples come from one fused
kernel (functional.tps_grid_sample) that evaluates the spline only at the at most 27 lattice nodes a sample depends on: no
lattice, no field.  `thin_plate_dense` still returns the field for callers that want it.  The reference's conventions are kept,
odd as they are: step = 4, lambd = 0.1; coordinates and displacements are normalised by [W-1, H-1, D-1] of img_shape = (D, H, W);
the lattice and the field are sized from shape = (W, H, D), so that grid_sample's x runs along an axis of D voxels; the sampled
displacements are un-normalised by [H-1, W-1, D-1].  Without an image shape 'tps' raises: the reference fails there too, and a
grid-free variant (the spline evaluated at the samples themselves) is out of scope.

`register_all` (:191-297) is the driver that turns a data set of meshes into the arrays `data_set_correspondences` consumes.
The reference rests it on open3d; here `TriangleMesh.sample_points_poisson_disk` is `mesh.Meshes.sample_points_poisson_disk`
(weighted sample elimination on the GPU, all meshes of one object in one call), `evaluate_registration` and
`correspondence_distance_heuristic` are the functions of those names below, the rigid step runs once for all instances and
the deformable step `pair_batch` (instance, object) pairs at a time.  It writes no files and draws no plots: the five pickled
objects and the rows of correspondences.csv come back in a dict.  Parity with open3d's sampler (its random stream, its heap
loop) is unpinned."""
import numbers

import numpy as np
import torch
from torch.nn import functional as F

from .. import functional as F_hip
from ..mesh import Meshes
from ..metrics import _device, _mesh_arrays

INTERPOLATION_MODES = ['knn', 'tps']
CHECK_EVERY = 5   # iterations between two looks of the host at the "any item still active" word
SOLVERS = ['lu', 'cholesky']   # the deformable M-step's M x M solve: torch.linalg.solve_ex | csrc/cholesky.hip
TPS_SOLVERS = ['lu', 'nullspace']   # the spline's solve: torch.linalg.solve | the null-space Cholesky route (csrc/tps_nullspace.hip)
TPS_STEP, TPS_LAMBDA = 4, 0.1   # point_cloud_registration.py:129: the lattice has a quarter of the resolution; the ridge of the fit


class TPS:
    """point_cloud_registration.py:24-67, the reference's signatures.  c (n,3) control points, f (n,C) their values (C <= 4),
    theta (n+4,C): n spline weights, then the affine rows; every method also takes a leading batch axis.  `fit` and `z` run on
    the kernels of csrc/tps.hip and need GPU tensors; theta is fp64 (the weights sum to zero and cancel by a factor of
    thousands in `z`), `z` returns fp32.  `d` and `u` are the plain formulas for callers that want them; the kernels do not
    go through them."""

    @staticmethod
    def fit(c, f, lambd=0., solver='lu'):
        return F_hip.tps_fit(c, f, lambd, solver=solver)

    @staticmethod
    def d(a, b):
        """pairwise distances (.., Na, Nb) as roots of sums of squared differences (the reference expands ra + rb - 2 ab)"""
        d2 = torch.zeros(*a.shape[:-1], b.shape[-2], dtype=a.dtype, device=a.device)
        for k in range(a.shape[-1]):   # one coordinate at a time: no (Na, Nb, 3) intermediate
            d2 += (a[..., :, None, k] - b[..., None, :, k]).square()
        return d2.sqrt()

    @staticmethod
    def u(r):
        return (r ** 2) * torch.log(r + 1e-6)

    @staticmethod
    def z(x, c, theta):
        return F_hip.tps_eval(x, c, theta)


def thin_plate_dense(x1, y1, shape, step, lambd=.0, unroll_step_size=2 ** 12, solver='lu'):
    """point_cloud_registration.py:70-89: the spline through values y1 (B,n,C) at control points x1 (B,n,3) in [-1,1]^3 (x along
    the last axis of `shape`), evaluated on the align_corners=True lattice (D//step, H//step, W//step) of shape = (D,H,W) and
    upsampled trilinearly (align_corners=True) -> the dense field (B,D,H,W,C) fp32.  The lattice nodes are implied (the kernel
    reads no coordinate tensor); the upsampling is torch's.  The reference fits x1[0] only; here every item of the batch gets
    its field.  `unroll_step_size` is accepted and ignored (the kernel needs no chunking).  For callers that want the field:
    `interpolate_displacements_tps` does not build it."""
    D, H, W = (int(s) for s in shape)
    if isinstance(step, bool) or not isinstance(step, int) or step < 1 or min(D, H, W) < step:
        raise ValueError(f"thin_plate_dense: step={step!r} must be a positive integer no larger than any axis of shape {tuple(shape)}")
    if x1.dim() != 3 or y1.dim() != 3:
        raise ValueError(f"thin_plate_dense: expected x1 (B,n,3) and y1 (B,n,C), got {tuple(x1.shape)} and {tuple(y1.shape)}")
    D1, H1, W1 = D // step, H // step, W // step
    with torch.no_grad():
        theta = F_hip.tps_fit(x1, y1, lambd, solver=solver)
        y2 = F_hip.tps_eval((D1, H1, W1), x1, theta)
        y2 = y2.view(-1, D1, H1, W1, y2.shape[-1]).permute(0, 4, 1, 2, 3)
        return F.interpolate(y2, (D, H, W), mode='trilinear', align_corners=True).permute(0, 2, 3, 4, 1)


def interpolate_displacements_tps(existing_points, values_at_existing_points, interpolation_points, img_shape, solver='lu'):
    """point_cloud_registration.py:119-133 for a batch: existing_points and values_at_existing_points (B,n,3),
    interpolation_points (B,Q,3) in voxel units of an image img_shape = (D,H,W) -> displacements (B,Q,3) fp32 (2-D inputs: a
    batch of one, returned 2-D).  The reference's conventions, see the module docstring; any Q, also 1 (the reference's
    squeeze() breaks there).  A sample outside the volume reads grid_sample's zero padding.  GPU tensors in, GPU tensor out.
    solver (one of TPS_SOLVERS) is handed to functional.tps_fit."""
    e, v, q = existing_points, values_at_existing_points, interpolation_points
    try:
        D, H, W = (int(s) for s in img_shape)
    except (TypeError, ValueError):
        raise ValueError(f"interpolate_displacements_tps: img_shape must be (D, H, W), got {img_shape!r}") from None
    if min(D, H, W) < TPS_STEP:
        raise ValueError(f"interpolate_displacements_tps: every axis of img_shape {(D, H, W)} must hold at least {TPS_STEP} voxels")
    for name, t in (("existing_points", e), ("values_at_existing_points", v), ("interpolation_points", q)):
        if not torch.is_tensor(t) or t.dim() not in (2, 3) or t.dim() != e.dim() or t.shape[-1] != 3 or not t.is_floating_point():
            raise ValueError(f"interpolate_displacements_tps: {name} must be a floating-point (points, 3) or (batch, points, 3) "
                             f"tensor like the others, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if e.shape != v.shape or e.shape[:-2] != q.shape[:-2]:
        raise ValueError(f"interpolate_displacements_tps: expected existing (..,n,3), values (..,n,3) and query (..,Q,3), got "
                         f"{tuple(e.shape)}, {tuple(v.shape)} and {tuple(q.shape)}")
    F_hip._need_gpu(e, v, q)
    with torch.no_grad():
        e, v, q = e.float(), v.float(), q.float()
        norm = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float32, device=e.device)
        normalize = lambda grid: (grid / norm) * 2   # noqa: E731  (no -1 for displacements)
        control = normalize(e) - 1
        theta = F_hip.tps_fit(control, normalize(v), TPS_LAMBDA, solver=solver)
        sampled = F_hip.tps_grid_sample(normalize(q) - 1, control, theta, size=(W, H, D), step=TPS_STEP)
        return (sampled * torch.tensor([H - 1, W - 1, D - 1], dtype=torch.float32, device=e.device)) / 2


def _as_tensor(a, name):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{name} must be a numpy array or a torch tensor, got {type(a).__name__}")
    if a.dim() not in (2, 3) or a.shape[-1] != 3 or a.shape[-2] < 1 or not a.is_floating_point():
        raise ValueError(f"{name} must be a floating-point (points, 3) or (batch, points, 3) array, got {tuple(a.shape)} {a.dtype}")
    return a


def _det3(m):
    return (m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1])
            - m[:, 0, 1] * (m[:, 1, 0] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 0])
            + m[:, 0, 2] * (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]))


class _Registration:
    """the EM loop and its on-device bookkeeping; subclasses supply `_prepare` and `_maximization`"""

    def __init__(self, X, Y, max_iterations=100, tolerance=1e-3, w=0., sigma2=None):
        self._numpy = isinstance(Y, np.ndarray)
        if isinstance(X, np.ndarray) != self._numpy:
            raise TypeError("X and Y must both be numpy arrays or both be torch tensors")
        X, Y = _as_tensor(X, "X"), _as_tensor(Y, "Y")
        if not self._numpy:
            F_hip._need_gpu(X, Y)
            if X.device != Y.device:
                raise ValueError(f"X is on {X.device}, Y on {Y.device}")
        self._squeeze = Y.dim() == 2
        B = 1 if self._squeeze else Y.shape[0]
        if X.dim() == 3 and X.shape[0] != B:
            raise ValueError(f"X holds {X.shape[0]} clouds, Y {B}")
        if isinstance(max_iterations, bool) or not isinstance(max_iterations, numbers.Integral) or max_iterations < 0:
            raise ValueError(f"max_iterations must be a non-negative integer, got {max_iterations!r}")
        if not isinstance(tolerance, numbers.Real) or not tolerance >= 0:
            raise ValueError(f"tolerance must be a non-negative number, got {tolerance!r}")
        if not isinstance(w, numbers.Real) or not 0 <= w < 1:
            raise ValueError(f"the outlier weight w must lie in [0, 1), got {w!r}")
        if sigma2 is not None:
            s2 = torch.as_tensor(sigma2, dtype=torch.float64).reshape(-1)
            if s2.numel() not in (1, B) or not bool((s2 > 0).all()):
                raise ValueError(f"sigma2 must be positive, one value or one per item, got {sigma2!r}")
        self.X, self.Y = X, Y
        self.max_iterations, self.tolerance, self.w, self._sigma2_init = int(max_iterations), float(tolerance), float(w), sigma2
        self.B, self.N, self.M = B, X.shape[-2], Y.shape[-2]
        self._ready = False

    # ---- state
    def _setup(self):
        dev = torch.device("cuda", torch.cuda.current_device()) if self._numpy else self.Y.device
        f64 = dict(dtype=torch.float64, device=dev)
        X = self.X.to(**f64)
        self._X = X if X.dim() == 3 else X[None]                      # (B or 1, N, 3)
        self._Y = self.Y.to(**f64).reshape(self.B, self.M, 3)
        self._X32 = self.X.to(dtype=torch.float32, device=dev).contiguous()   # keeps (N,3): the kernel shares one cloud
        if self._X32.dim() == 3 and self.B == 1:
            self._X32 = self._X32[0]
        if self._sigma2_init is None:
            # sum_nm |x_n - y_m|^2 = M sum |x|^2 + N sum |y|^2 - 2 (sum x).(sum y), in fp64
            sx, sy = self._X.sum(1), self._Y.sum(1)
            tot = self.M * self._X.square().sum((1, 2)) + self.N * self._Y.square().sum((1, 2)) - 2 * (sx * sy).sum(1)
            self._sigma2 = (tot / (3 * self.N * self.M)).expand(self.B).clone()
        else:
            self._sigma2 = torch.as_tensor(self._sigma2_init, **f64).reshape(-1).expand(self.B).clone()
        self._TY = self._Y.clone()
        self._active = torch.full((self.B,), self.max_iterations > 0, dtype=torch.bool, device=dev)
        self._iters = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._prepare(dev)
        self._ready = True

    def _keep(self, new, old):
        """`new` for the active items, `old` for the frozen ones"""
        return torch.where(self._active.view(-1, *([1] * (new.dim() - 1))), new, old)

    def _finish_iteration(self, sigma2, diff):
        floor = torch.full_like(sigma2, self.tolerance / 10)
        self._sigma2 = self._keep(torch.where(sigma2 > 0, sigma2, floor), self._sigma2)
        self._iters += self._active
        self._active = self._active & (diff > self.tolerance)

    def _expectation(self):
        return [t.double() for t in F_hip.cpd_estep(self._X32, self._TY.float(), self._sigma2.float(), self.w)]

    def register(self):
        with torch.no_grad():
            self._setup()   # every call registers from the start
            for it in range(self.max_iterations):
                if it and it % CHECK_EVERY == 0 and not bool(self._active.any()):   # the only synchronisation of the loop
                    break
                self._maximization(*self._expectation())
            self._check_run()
            return self._out(self._TY), self.get_registration_parameters()

    def _check_run(self):
        """what a subclass has to look at once the loop is through (the one place it may read the device)"""

    # ---- results
    def _out(self, t):
        t = t.to(self.Y.dtype)
        if self._squeeze:
            t = t[0]
        return t.cpu().numpy() if self._numpy else t

    @property
    def iteration(self):
        """EM iterations each item ran: an int for a 2-D Y, else (B,)"""
        if not self._ready:
            return 0 if self._squeeze else self._out_int(torch.zeros(self.B, dtype=torch.int32))
        return int(self._iters[0]) if self._squeeze else self._out_int(self._iters.clone())

    def _out_int(self, t):
        return t.cpu().numpy() if self._numpy else t

    @property
    def sigma2(self):
        return self._out(self._sigma2) if self._ready else None

    @property
    def TY(self):
        return self._out(self._TY) if self._ready else None


class RigidRegistration(_Registration):
    """Rigid CPD with scaling (Myronenko & Song fig. 2): `register()` -> (TY, (scale, rotation, translation)) with
    TY = scale * Y @ rotation + translation -- the row-vector convention the reference relies on
    (point_cloud_registration.py:232-237; it stores rotation.T for the column-vector form)."""

    def _prepare(self, dev):
        B = self.B
        self._s = torch.ones(B, dtype=torch.float64, device=dev)
        self._R = torch.eye(3, dtype=torch.float64, device=dev).expand(B, 3, 3).clone()   # paper's R: T(y) = s R y + t
        self._t = torch.zeros(B, 3, dtype=torch.float64, device=dev)
        self._q = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)

    def _maximization(self, P1, Pt1, PX, Np):
        X, Y = self._X, self._Y
        muX = PX.sum(1) / Np[:, None]
        muY = (P1[:, :, None] * Y).sum(1) / Np[:, None]
        Xh, Yh = X - muX[:, None], Y - muY[:, None]
        A = (PX - P1[:, :, None] * muX[:, None]).transpose(1, 2) @ Yh          # X^T P^T Y, centred: (B,3,3)
        U, _, Vh = torch.linalg.svd(A)
        C = torch.ones_like(muX)
        C[:, 2] = _det3(U) * _det3(Vh)
        R = (U * C[:, None, :]) @ Vh
        trAR = (A * R).sum((1, 2))                                              # tr(A^T R)
        yPy = (P1 * Yh.square().sum(2)).sum(1)
        xPx = (Pt1 * Xh.square().sum(2)).sum(1)
        s = trAR / yPy
        t = muX - s[:, None] * (R @ muY[:, :, None]).squeeze(2)
        TY = s[:, None, None] * (Y @ R.transpose(1, 2)) + t[:, None]
        q = (xPx - 2 * s * trAR + s * s * yPy) / (2 * self._sigma2) + 1.5 * Np * torch.log(self._sigma2)
        diff = (q - self._q).abs()
        self._s, self._R, self._t = self._keep(s, self._s), self._keep(R, self._R), self._keep(t, self._t)
        self._TY, self._q = self._keep(TY, self._TY), self._keep(q, self._q)
        self._finish_iteration((xPx - s * trAR) / (3 * Np), diff)

    def get_registration_parameters(self):
        s, rot, t = self._s, self._R.transpose(1, 2).contiguous(), self._t
        if self._squeeze and self._numpy:
            return float(s[0]), self._out(rot), self._out(t)
        return self._out(s), self._out(rot), self._out(t)


class DeformableRegistration(_Registration):
    """Non-rigid CPD (Myronenko & Song fig. 4): `register()` -> (TY, (G, W)) with TY = Y + G @ W,
    G[i,j] = exp(-|y_i - y_j|^2 / (2 beta^2)).  `alpha` weighs the smoothness of the displacement field against the point
    fit, `beta` is the width of the kernel that defines smoothness.  G and the solve are fp64.  `solver`: 'lu' (default) solves
    the M x M system with torch.linalg.solve_ex; 'cholesky' solves its symmetric positive definite form on the kernels of
    csrc/cholesky.hip (module docstring) and raises RuntimeError at the end of `register()` if a system was rejected."""

    def __init__(self, X, Y, alpha, beta, max_iterations=100, tolerance=1e-3, w=0., sigma2=None, solver='lu'):
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        self.solver = solver
        super().__init__(X, Y, max_iterations=max_iterations, tolerance=tolerance, w=w, sigma2=sigma2)
        for name, v in (("alpha", alpha), ("beta", beta)):
            if not isinstance(v, numbers.Real) or not v > 0:
                raise ValueError(f"{name} must be a positive number, got {v!r}")
        self.alpha, self.beta = float(alpha), float(beta)

    def _prepare(self, dev):
        Y = self._Y
        d = torch.zeros(self.B, self.M, self.M, dtype=torch.float64, device=dev)
        for c in range(3):   # differences, one coordinate at a time: no (B,M,M,3) intermediate
            d += (Y[:, :, None, c] - Y[:, None, :, c]).square()
        self._G = torch.exp(d.mul_(-1 / (2 * self.beta ** 2)))
        self._W = torch.zeros(self.B, self.M, 3, dtype=torch.float64, device=dev)
        self._eye = torch.eye(self.M, dtype=torch.float64, device=dev)
        self._info = torch.zeros(self.B, dtype=torch.int32, device=dev)   # 'cholesky': the largest status over the iterations
        self._Xsq = self._X.square().sum(2)

    def _maximization(self, P1, Pt1, PX, Np):
        Y, G = self._Y, self._G
        if self.solver == 'cholesky':
            S, rhs, d = F_hip.cpd_spd_system(G, P1, PX, Y, self._sigma2, self.alpha)
            V, info = F_hip.spd_solve(S, rhs, overwrite=True)
            self._info = torch.maximum(self._info, info)              # stays on the device: the loop stays asynchronous
            W = d[:, :, None] * V
        else:
            A = P1[:, :, None] * G + (self.alpha * self._sigma2)[:, None, None] * self._eye
            W = torch.linalg.solve_ex(A, PX - P1[:, :, None] * Y)[0]   # no status read-back: the loop stays asynchronous
        TY = Y + G @ W
        xPx = (Pt1 * self._Xsq).sum(1)
        yPy = (P1 * TY.square().sum(2)).sum(1)
        trPXY = (TY * PX).sum((1, 2))
        sigma2 = (xPx - 2 * trPXY + yPy) / (3 * Np)
        floor = torch.full_like(sigma2, self.tolerance / 10)
        diff = (torch.where(sigma2 > 0, sigma2, floor) - self._sigma2).abs()
        self._W, self._TY = self._keep(W, self._W), self._keep(TY, self._TY)
        self._finish_iteration(sigma2, diff)

    def _check_run(self):
        if self.solver == 'cholesky':
            bad = self._info.nonzero().flatten().tolist()
            if bad:
                raise RuntimeError(f"DeformableRegistration(solver='cholesky'): the M-step system of item(s) {bad} was not positive "
                                   f"definite in some iteration (status {self._info[bad].tolist()}); solver='lu' takes such input")

    def get_registration_parameters(self):
        return self._out(self._G), self._out(self._W)

    def displacements(self):
        """G @ W = TY - Y, formed in fp64 before it is cast to the type of Y"""
        return self._out(self._G @ self._W)


def register_cpd_deformable(fixed_pc_np, moving_pc_np_prereg, solver='lu'):
    """point_cloud_registration.py:101-116 (assumes a rigid / affine pre-registration): deformable CPD with alpha = 0.01,
    beta = 10 -> (deformed cloud, its displacements G @ W).  Batched inputs register every pair at once.  `solver`: as in
    DeformableRegistration."""
    deformable = DeformableRegistration(X=fixed_pc_np, Y=moving_pc_np_prereg, alpha=0.01, beta=10, solver=solver)
    deformed, _ = deformable.register()
    return deformed, deformable.displacements()


def interpolate_displacements_weighted_knn(existing_points, values_at_existing_points, interpolation_points, k=5):
    """point_cloud_registration.py:136-148: at every interpolation point, the mean of the values at its k nearest existing
    points, weighted by 1 / (distance + 1e-8).  existing_points (Ne,3) or (B,Ne,3), values (.., Ne, C), interpolation_points
    (.., Nq, 3) -> (.., Nq, C) fp32.  The neighbours come from the segment kNN kernel and the weighted mean from the
    interpolation kernel of the PointTransformer (functional.knn_segment / functional.interpolate); no (Nq, Ne) distance
    matrix, no dense topk.  GPU tensors in, GPU tensor out (the reference returns a squeezed numpy array)."""
    e, v, q = existing_points, values_at_existing_points, interpolation_points
    F_hip._need_gpu(e, v, q)
    if e.dim() not in (2, 3) or e.dim() != v.dim() or e.dim() != q.dim() or e.shape[-1] != 3 or q.shape[-1] != 3 \
            or e.shape[:-1] != v.shape[:-1] or e.shape[:-2] != q.shape[:-2]:
        raise ValueError(f"expected existing (..,Ne,3), values (..,Ne,C) and query (..,Nq,3), got {tuple(e.shape)}, "
                         f"{tuple(v.shape)} and {tuple(q.shape)}")
    Ne, Nq, C = e.shape[-2], q.shape[-2], v.shape[-1]
    if not 1 <= k <= min(8, Ne):
        raise ValueError(f"k={k}: the interpolation kernel serves 1 <= k <= 8, and k <= {Ne} existing points")
    B = e.shape[0] if e.dim() == 3 else 1
    with torch.no_grad():
        offset = torch.arange(1, B + 1, dtype=torch.int32, device=e.device)
        idx, d2 = F_hip.knn_segment(k, e.reshape(B * Ne, 3), q.reshape(B * Nq, 3), offset * Ne, offset * Nq)
        out = F_hip.interpolate(v.reshape(B * Ne, C), idx, d2)
    return out.view(*q.shape[:-1], C)


TPS_NEEDS_SHAPE = ("{}(interpolation_mode='tps') without {}: the thin-plate-spline interpolation samples a displacement field on the "
                   "image grid, and a grid-free variant is out of scope of this package; pass the image shape (D, H, W) or use 'knn'")


def inverse_transformation_at_sampled_points(deformed_pc_np, moving_displacements, sample_point_cloud, img_shape=None,
                                             interpolation_mode='knn', tps_solver='lu'):
    """point_cloud_registration.py:151-177: the displacements of the moved cloud, interpolated at the sample locations and
    subtracted from them -> the sample points in the moving cloud's space.  numpy in, numpy out (as the reference); GPU
    tensors in, GPU tensor out.  'knn' needs no image shape; 'tps' needs img_shape = (D, H, W) and raises without it; tps_solver
    (one of TPS_SOLVERS) is the solve of its fit."""
    if interpolation_mode not in INTERPOLATION_MODES:
        raise ValueError(f"interpolation_mode must be one of {INTERPOLATION_MODES}, got {interpolation_mode!r}")
    if interpolation_mode == 'tps' and img_shape is None:
        raise NotImplementedError(TPS_NEEDS_SHAPE.format("inverse_transformation_at_sampled_points", "img_shape"))
    as_numpy = isinstance(sample_point_cloud, np.ndarray)
    if as_numpy:
        dev = torch.device("cuda", torch.cuda.current_device())
        deformed, disp, sample = (torch.from_numpy(np.asarray(a)).to(device=dev, dtype=torch.float32)
                                  for a in (deformed_pc_np, moving_displacements, sample_point_cloud))
    else:
        deformed, disp, sample = deformed_pc_np, moving_displacements, sample_point_cloud
    if interpolation_mode == 'tps':
        interpolated = interpolate_displacements_tps(deformed, disp, sample, img_shape, solver=tps_solver)
    else:
        interpolated = interpolate_displacements_weighted_knn(deformed, disp, sample)
    if as_numpy:
        return sample_point_cloud - interpolated.cpu().numpy().astype(sample_point_cloud.dtype)
    return sample - interpolated.to(sample.dtype)


# ------------------------------------------------------------------ the driver (point_cloud_registration.py:180-297)
def correspondence_distance_heuristic(pc):
    """point_cloud_registration.py:180-188: 5 % of the longest diagonal through the bounding box of a cloud (N,3) -- a float for
    numpy, a 0-d tensor for a tensor -- or of every cloud of a batch (B,N,3) -> (B,)."""
    if isinstance(pc, np.ndarray):
        if pc.ndim not in (2, 3) or pc.shape[-1] != 3 or pc.shape[-2] < 1:
            raise ValueError(f"pc must be (points, 3) or (batch, points, 3), got {pc.shape}")
        diag = np.linalg.norm(pc.max(-2) - pc.min(-2), ord=2, axis=-1)
        return diag.item() * 0.05 if pc.ndim == 2 else diag * 0.05
    pc = _as_tensor(pc, "pc")
    return torch.linalg.vector_norm(pc.amax(-2) - pc.amin(-2), ord=2, dim=-1) * 0.05


def evaluate_registration(source, target, max_correspondence_distance):
    """open3d.pipelines.registration.evaluate_registration without a transformation, batched through functional.chamfer_nn:
    source (N,3) or (B,N,3), target (M,3) or (B,M,3), max_correspondence_distance a number or (B,) -> dict with
    `n_correspondences`, the number of source points whose nearest target point lies within the distance (<=; the length of
    open3d's correspondence_set), `fitness` = that count / N and `inlier_rmse`, the root mean square of those nearest
    distances (0 without inliers).  The nearest squared distance is the kernel's fp32 value; its root is compared in fp64.
    numpy in, numpy out (Python numbers for a 2-D source); GPU tensors in, GPU tensors out."""
    as_numpy = isinstance(source, np.ndarray)
    if isinstance(target, np.ndarray) != as_numpy:
        raise TypeError("source and target must both be numpy arrays or both be torch tensors")
    src, tgt = _as_tensor(source, "source"), _as_tensor(target, "target")
    squeeze = src.dim() == 2
    if tgt.dim() != src.dim():
        raise ValueError(f"source {tuple(src.shape)} and target {tuple(tgt.shape)} must both be single clouds or both batches")
    if squeeze:
        src, tgt = src[None], tgt[None]
    B, N = src.shape[0], src.shape[1]
    if tgt.shape[0] != B:
        raise ValueError(f"source holds {B} clouds, target {tgt.shape[0]}")
    if not as_numpy:
        F_hip._need_gpu(src, tgt)
    dev = _device() if as_numpy else src.device
    with torch.no_grad():
        limit = torch.as_tensor(max_correspondence_distance, dtype=torch.float64).to(dev).reshape(-1)
        if limit.numel() not in (1, B):
            raise ValueError(f"max_correspondence_distance must be one value or one per cloud ({B}), got {limit.numel()}")
        d2, _ = F_hip.chamfer_nn(src.to(device=dev, dtype=torch.float32).contiguous(),
                                 tgt.to(device=dev, dtype=torch.float32).contiguous())
        d2 = d2.detach().double()
        inlier = d2.sqrt() <= limit[:, None]
        count = inlier.sum(1)
        rmse = torch.where(count > 0, ((d2 * inlier).sum(1) / count.clamp(min=1)).sqrt(), torch.zeros_like(limit.expand(B)))
        # (a tensor divisor: torch divides by a Python number through its reciprocal, which is not count / N to the last bit)
        out = {"n_correspondences": count, "fitness": count.double() / torch.full_like(rmse, N), "inlier_rmse": rmse}
    if squeeze:
        out = {k: v[0] for k, v in out.items()}
    if as_numpy:
        out = {k: (v.item() if squeeze else v.cpu().numpy()) for k, v in out.items()}
    return out


def _fixed_clouds(fixed_pcs):
    """a sequence of (P,3) clouds or an (objects, P, 3) array -> (as_numpy, list of per-object arrays / tensors); ragged
    objects are refused before anything runs"""
    clouds = list(fixed_pcs)
    if not clouds:
        raise ValueError("register_all: no fixed point clouds")
    as_numpy = not torch.is_tensor(clouds[0])
    if as_numpy:
        clouds = [np.asarray(c) for c in clouds]
    elif not all(torch.is_tensor(c) for c in clouds):
        raise TypeError("register_all: fixed_pcs must be all numpy arrays or all torch tensors")
    for c in clouds:
        if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1:
            raise ValueError(f"register_all: a fixed cloud must be (points, 3), got {tuple(c.shape)}")
    counts = [int(c.shape[0]) for c in clouds]
    if len(set(counts)) != 1:
        raise ValueError(f"register_all: the fixed clouds of the objects hold {counts} points; every object must hold the same "
                         f"number (data_set_correspondences needs equal counts)")
    return as_numpy, clouds


def register_all(fixed_pcs, all_moving_meshes, ids=None, base_dir=None, n_sample_points=1024, show=False, generator=None,
                 pair_batch=32, solver='lu'):
    """point_cloud_registration.py:191-297.  fixed_pcs: one (P,3) cloud per object (a sequence or an (objects, P, 3) array);
    all_moving_meshes[instance][object]: a mesh in any form `metrics._mesh_arrays` takes (a (verts, faces) pair, an open3d
    TriangleMesh); surplus objects of an instance are dropped as in the reference.  Steps:
      1. every moving mesh is sampled to P points with `Meshes.sample_points_poisson_disk` -- the meshes of one object over all
         instances in one call, objects in order, all drawing from `generator`;
      2. ONE batched RigidRegistration of the concatenated objects (fixed: shared, moving: one row per instance);
      3. the result is split per object and registered with `register_cpd_deformable`, `pair_batch` (instance, object) pairs
         at a time in instance-major order (the M x M fp64 systems of a chunk set the memory), with the M-step `solver` of
         DeformableRegistration ('lu' | 'cholesky');
      4. `evaluate_registration` of every deformed cloud (as fp32, like the reference) against its fixed cloud within
         `correspondence_distance_heuristic` of that fixed cloud.
    -> dict: `displacements`, `moved_pcs`, `moving_pcs` (instances, objects, P, 3) fp64; `transforms`, one dict per instance
    with `scale`, `translation` and `rotation` (transposed to the column-vector form A x, :237); `ids`;
    `n_correspondences` and `corr_distances` (instances, objects); `correspondences`, the rows of the reference's
    correspondences.csv as a dict of lists (per object, then the overall value; numpy's population std).
    numpy in, numpy out; GPU tensors in, GPU tensors out.  `base_dir`, `show` and `n_sample_points` are accepted and ignored
    (no files, no plots; the reference does not use n_sample_points either).  The first four arrays feed
    `data_set_correspondences(fixed_pcs, all_moving_meshes, out['moving_pcs'], out['transforms'], out['moved_pcs'],
    out['displacements'], mode=...)` unchanged."""
    as_numpy, clouds = _fixed_clouds(fixed_pcs)
    O, P = len(clouds), int(clouds[0].shape[0])
    all_moving_meshes = [list(m)[:O] for m in all_moving_meshes]
    I = len(all_moving_meshes)
    if I == 0 or any(len(m) != O for m in all_moving_meshes):
        raise ValueError(f"register_all: every instance must hold a mesh for each of the {O} objects")
    ids = list(range(I)) if ids is None else list(ids)
    if len(ids) != I:
        raise ValueError(f"register_all: {len(ids)} ids for {I} instances")
    if isinstance(pair_batch, bool) or not isinstance(pair_batch, int) or pair_batch < 1:
        raise ValueError(f"register_all: pair_batch must be a positive integer, got {pair_batch!r}")
    if solver not in SOLVERS:
        raise ValueError(f"register_all: solver must be one of {SOLVERS}, got {solver!r}")
    if not as_numpy:
        F_hip._need_gpu(*clouds)
    dev = _device() if as_numpy else clouds[0].device
    with torch.no_grad():
        fixed = torch.stack([(torch.from_numpy(np.ascontiguousarray(c)) if as_numpy else c).to(device=dev, dtype=torch.float64)
                             for c in clouds])                                                       # (O, P, 3)
        moving = []
        for obj in range(O):
            arrays = [_mesh_arrays(m[obj]) for m in all_moving_meshes]
            meshes = Meshes([v.to(dev) for v, _ in arrays], [f.to(dev) for _, f in arrays])
            moving.append(meshes.sample_points_poisson_disk(P, generator=generator))
        moving = torch.stack(moving, 1).double()                                                     # (I, O, P, 3)

        rigid = RigidRegistration(X=fixed.reshape(O * P, 3), Y=moving.reshape(I, O * P, 3))
        prereg, (scale, rotation, translation) = rigid.register()
        rotation = rotation.transpose(1, 2).contiguous()

        X = fixed[None].expand(I, O, P, 3).reshape(I * O, P, 3)
        Y = prereg.reshape(I * O, P, 3)
        moved, disp = [], []
        for p0 in range(0, I * O, pair_batch):
            deformed, d = register_cpd_deformable(X[p0:p0 + pair_batch].contiguous(), Y[p0:p0 + pair_batch].contiguous(),
                                                  solver=solver)
            moved.append(deformed)
            disp.append(d)
        moved, disp = torch.cat(moved), torch.cat(disp)

        corr_dist = correspondence_distance_heuristic(fixed)                                         # (O,)
        corr_distances = corr_dist[None].expand(I, O)
        found = evaluate_registration(moved.float(), X.float(), corr_distances.reshape(-1))
        n_corr = found["n_correspondences"].reshape(I, O)

    n_host, dist_host = n_corr.cpu().numpy(), corr_distances.cpu().numpy()
    portion = n_host / float(P)
    rows = {"Object No.": [str(obj + 1) for obj in range(O)] + ["mean"],
            "Mean corresponding": portion.mean(0).tolist() + [portion.mean().item()],
            "StdDev corresponding": portion.std(0).tolist() + [portion.std().item()],
            "Max. corr dist": dist_host.mean(0).tolist() + [dist_host.mean().item()]}
    out = {"displacements": disp.reshape(I, O, P, 3), "moved_pcs": moved.reshape(I, O, P, 3), "moving_pcs": moving,
           "n_correspondences": n_corr, "corr_distances": corr_distances.contiguous()}
    if as_numpy:
        out = {k: v.cpu().numpy() for k, v in out.items()}
        s, R, t = scale.cpu().numpy(), rotation.cpu().numpy(), translation.cpu().numpy()
        out["transforms"] = [{"scale": float(s[i]), "translation": t[i], "rotation": R[i]} for i in range(I)]
    else:
        out["transforms"] = [{"scale": scale[i], "translation": translation[i], "rotation": rotation[i]} for i in range(I)]
    out["ids"] = np.asarray(ids)
    out["correspondences"] = rows
    return out
