"""The DPSR front (point cloud <-> grid, spectral Poisson solve, DPSR, the SoftMesh field) restated in plain torch: seeded
inputs for tests/golden/dpsr_*.npz (tools/make_golden_dpsr.py stores only the reference's outputs for them) and an oracle that
runs in fp64 or fp32, on any device, with torch's autograd for every gradient.

Conventions (csrc/grid_points.hip has the same text): 'torch' = F.grid_sample(mode='bilinear', padding_mode='zeros',
align_corners=False), coords (x -> W, y -> H, z -> D) in [-1, 1]; 'sap' = point_rasterize / grid_interp, coords (0 -> D, 1 -> H,
2 -> W) in [0, 1], cubesize 1 / (size - 1).  In 'sap' mode the INDICES are always taken from the fp32 expressions (they are
constants of the method: which voxel a node point reaches is decided by fp32 rounding), the weights in the oracle's dtype."""
import math

import numpy as np
import torch
import torch.nn.functional as F

GRID = (8, 10, 12)          # D, H, W of the small cases: no two axes alike
RES = (16, 16, 16)
SIG = 2.0
SMOOTH_SIGMA = 2.0
# seeds of the random clouds whose coordinate gradients are compared: chosen so that no point lies within 1e-3 of a cell of a
# node plane (far_from_planes), where the gradient jumps.  (mode, C) -> seed for B = 2, N = 50 on GRID
SEEDS = {("torch", 3): 6, ("sap", 3): 8, ("torch", 1): 21, ("sap", 1): 21, ("torch", 5): 25, ("sap", 5): 25}
SEED_N1 = 60
RANGE = {"torch": (-1.2, 1.2), "sap": (0.0, 1.0)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ seeded inputs (CPU fp32)
def cloud_case(seed, B=2, C=3, N=50, lo=-1.2, hi=1.2, size=GRID):
    """values (B, C, N), coords (B, N, 3) uniform in [lo, hi], g_grid (B, C, *size), g_pts (B, C, N), grid (B, C, *size)"""
    g = _gen(seed)
    return dict(values=torch.randn(B, C, N, generator=g), coords=torch.rand(B, N, 3, generator=g) * (hi - lo) + lo,
                g_grid=torch.randn(B, C, *size, generator=g), g_pts=torch.randn(B, C, N, generator=g),
                grid=torch.randn(B, C, *size, generator=g))


def leaf(t, dtype=None, device=None):
    """a fresh leaf in the given dtype / device (never the stored input itself)"""
    return t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)


def clear_coords(mode, size, B, N, seed, margin=0.01):
    """a random cloud whose cell coordinates keep `margin` of a cell from every node plane (for shapes too large to get that
    from the choice of a seed): cell = integer + margin + (1 - 2 margin) u, over the whole coordinate range of RANGE[mode]"""
    g = _gen(seed)
    cols = []
    for S in (size[::-1] if mode == "torch" else size):
        lo, hi = (-0.1 * S - 0.5, 1.1 * S - 0.5) if mode == "torch" else (0.0, S - 1.0)
        k = torch.floor(torch.rand(B, N, generator=g, dtype=torch.float64) * (hi - lo) + lo)
        t = (k + margin + (1 - 2 * margin) * torch.rand(B, N, generator=g, dtype=torch.float64)).clamp(lo + margin, hi - margin)
        cols.append((2 * t + 1) / S - 1 if mode == "torch" else t / (S - 1))
    return torch.stack(cols, -1).float()


def node_coords(mode, size=GRID):
    """points exactly on voxel centres / nodes (every combination along the diagonal and the extremes) plus the ends of the
    coordinate range -> (1, N, 3) fp32"""
    D, H, W = size
    n = max(size)
    i = torch.arange(n, dtype=torch.float64)
    if mode == "torch":      # voxel centre i of an axis of S voxels: (2 i + 1) / S - 1
        cols = [(2 * (i % S) + 1) / S - 1 for S in (W, H, D)]
        ends = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]
    else:                    # node i of an axis of S nodes: i / (S - 1)
        cols = [(i % S) / (S - 1) for S in (D, H, W)]
        ends = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.5], [1.0, 0.0, 0.25]]
    pts = torch.cat([torch.stack(cols, 1), torch.tensor(ends, dtype=torch.float64)])
    mixed = pts.clone()      # a node coordinate on one axis only
    mixed[:, 1] = 0.3137
    return torch.cat([pts, mixed]).float()[None]


def one_cell_coords(mode, N=2048, seed=5, size=(128, 128, 128), cell=40):
    """N points inside cell `cell` (on every axis) of a grid -> (1, N, 3)"""
    u = torch.rand(1, N, 3, generator=_gen(seed), dtype=torch.float64) * 0.8 + 0.1
    S = torch.tensor(size[::-1] if mode == "torch" else size, dtype=torch.float64)
    return ((2 * (cell + u) + 1) / S - 1 if mode == "torch" else (cell + u) / (S - 1)).float()


def sphere_case(seed=11, B=2, N=200):
    """points on a sphere of radius 0.5 with outward normals (a well-conditioned |phi[0, 0, 0]|) and the test loss's weights"""
    g = _gen(seed)
    n = F.normalize(torch.randn(B, N, 3, generator=g), dim=-1)
    return dict(V=0.5 * n, N=n.clone(), g_phi=torch.randn(B, *RES, generator=g))


def softmesh_case(seed=12, B=2, K=3, N=300):
    """spatially coherent logits: the two foreground classes trade places along x (a mild ramp), the background is constant.
    SoftMesh splats coords in grid_sample's convention and then reads THE SAME numbers in the [0, 1] convention
    (seg_logits_to_mesh.py:95, :108-109), so the cloud sits in [0.75, 1): there the two placements overlap and the mean of the
    field over the points differs from phi[0, 0, 0] (|phi0| / max |phi| is 0.2 - 0.35; a cloud spread over [0.1, 0.9] gave 0.05)
    -> logits (B, K, N), coords (B, 3, N), g_field"""
    g = _gen(seed)
    lo, hi = 0.75, 1.0
    coords = torch.rand(B, 3, N, generator=g) * (hi - lo) + lo
    u = (coords[:, 0] - (lo + hi) / 2) / ((hi - lo) / 2)
    logits = torch.stack([torch.full_like(u, -1.0)] + [u * (1.0 if k % 2 == 0 else -1.0) for k in range(1, K)], 1)
    return dict(logits=logits, coords=coords, g_field=torch.randn(B * (K - 1), *RES, generator=g))


# ------------------------------------------------------------------ the oracle
def _axis(x, S, mode):
    """one memory axis: (lower index, upper index, their weights); x (B, N) in the oracle's dtype"""
    if mode == "torch":
        t = ((x + 1) * S - 1) / 2
        f = torch.floor(t.detach())
        return f.long(), f.long() + 1, (f + 1) - t, t - f
    p32 = x.detach().float()
    size32 = torch.tensor(float(S), dtype=torch.float32, device=x.device)
    cs32 = 1.0 / (size32 - 1)
    t32 = p32 / cs32
    f0 = torch.floor(t32)
    i1 = torch.fmod(torch.ceil(t32), size32).long()
    cs = 1.0 / torch.tensor(float(S) - 1, dtype=x.dtype, device=x.device)
    f0d = f0.to(x.dtype)
    return f0.long(), i1, torch.abs(x - (f0d + 1) * cs) / cs, torch.abs(x - f0d * cs) / cs


def corners(coords, size, mode):
    """-> idx (B, N, 8) int64 linear voxel (D H W where the corner is outside), w (B, N, 8) differentiable in coords"""
    D, H, W = size
    comp = (2, 1, 0) if mode == "torch" else (0, 1, 2)          # coordinate component of memory axes D, H, W
    ax = [_axis(coords[..., c], S, mode) for c, S in zip(comp, size)]
    idx, w = [], []
    for k in range(8):
        pick = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
        i = [a[p] for a, p in zip(ax, pick)]
        ww = [a[2 + p] for a, p in zip(ax, pick)]
        ok = (i[0] >= 0) & (i[0] < D) & (i[1] >= 0) & (i[1] < H) & (i[2] >= 0) & (i[2] < W)
        idx.append(torch.where(ok, (i[0] * H + i[1]) * W + i[2], torch.full_like(i[0], D * H * W)))
        w.append(ww[0] * ww[1] * ww[2])
    return torch.stack(idx, -1), torch.stack(w, -1)


def splat(values, coords, size, mode):
    """values (B, C, N), coords (B, N, 3) -> (B, C, D, H, W)"""
    B, C, N = values.shape
    DHW = size[0] * size[1] * size[2]
    idx, w = corners(coords, size, mode)
    contrib = (values[..., None] * w[:, None]).reshape(B, C, N * 8)
    out = torch.zeros(B, C, DHW + 1, dtype=values.dtype, device=values.device)
    out = out.scatter_add(2, idx.reshape(B, 1, N * 8).expand(B, C, N * 8), contrib)
    return out[..., :DHW].reshape(B, C, *size)


def sample(grid, coords, mode):
    """grid (B, C, D, H, W), coords (B, N, 3) -> (B, C, N)"""
    B, C = grid.shape[:2]
    size = tuple(grid.shape[2:])
    N = coords.shape[1]
    idx, w = corners(coords, size, mode)
    flat = torch.cat([grid.reshape(B, C, -1), torch.zeros(B, C, 1, dtype=grid.dtype, device=grid.device)], 2)
    vals = flat.gather(2, idx.reshape(B, 1, N * 8).expand(B, C, N * 8)).reshape(B, C, N, 8)
    return (vals * w[:, None]).sum(-1)


def far_from_planes(coords, size, mode, margin=1e-3):
    """(B, N) bool: every coordinate at least `margin` of a cell from every node plane (where the coordinate gradient jumps)"""
    c = coords.double()
    comp = (2, 1, 0) if mode == "torch" else (0, 1, 2)
    ok = torch.ones(c.shape[:2], dtype=torch.bool, device=c.device)
    for ci, S in zip(comp, size):
        t = ((c[..., ci] + 1) * S - 1) / 2 if mode == "torch" else c[..., ci] * (S - 1)
        ok &= (t - torch.round(t)).abs() >= margin
    return ok


def freqs(res, dtype, device):
    """(R0, R1, R2 / 2 + 1, 3) integer frequencies of rfftn over res"""
    f = [torch.tensor(np.fft.fftfreq(r, d=1 / r), dtype=dtype, device=device) for r in res[:2]]
    f.append(torch.tensor(np.fft.rfftfreq(res[2], d=1 / res[2]), dtype=dtype, device=device))
    return torch.stack(torch.meshgrid(*f, indexing="ij"), -1)


def spectral(nhat, res, sig):
    """nhat (B, 3, R0, R1, R2 / 2 + 1) complex -> Phi (B, R0, R1, R2 / 2 + 1)"""
    real = torch.float64 if nhat.dtype == torch.complex128 else torch.float32
    f64 = freqs(res, torch.float64, nhat.device)
    G = torch.exp(-0.5 * (sig * 2 * f64.pow(2).sum(-1).sqrt() / res[0]) ** 2).to(real)
    om = freqs(res, real, nhat.device) * (2 * math.pi)
    div = sum(-1j * om[..., d] * (nhat[:, d] * G) for d in range(3))
    Phi = div / (-(om ** 2).sum(-1) + 1e-6)
    mask = torch.ones(Phi.shape[1:], dtype=real, device=nhat.device)
    mask[0, 0, 0] = 0
    return Phi * mask


def psr_field(V01, field, res, sig, shift=True, scale=True, prescale=False):
    """spectral_PSR: V01 (B, N, 3) in [0, 1], field (B, 3, *res) -> phi (B, *res)"""
    phi = torch.fft.irfftn(spectral(torch.fft.rfftn(field, dim=(2, 3, 4)), res, sig), s=res, dim=(1, 2, 3))
    if shift:
        phi = phi - sample(phi[:, None], V01, "sap")[:, 0].mean(-1).view(-1, 1, 1, 1)
    if prescale:
        return phi
    if scale:
        phi = -phi / phi[:, 0, 0, 0].abs().view(-1, 1, 1, 1) * 0.5
    return phi


def dpsr(V, N, res=RES, sig=SIG, **kw):
    """DPSR.forward: V (B, n, 3) in [-1, 1], N normals -> phi (B, *res)"""
    V01 = (V + 1) / 2
    return psr_field(V01, splat(N.transpose(1, 2), V01, res, "sap"), res, sig, **kw)


def derivative_taps(sigma, order, truncate, dtype=torch.float64):
    """Gaussian (order 0), its first and second derivative, sampled at the integers and normalised by the Gaussian's sum"""
    r = int(truncate * float(sigma) + 0.5)
    x = torch.arange(-r, r + 1, dtype=torch.float64)
    phi = torch.exp(-x ** 2 / (2 * sigma ** 2))
    phi = phi / phi.sum()
    poly = {0: torch.ones_like(x), 1: -x / sigma ** 2, 2: x ** 2 / sigma ** 4 - 1 / sigma ** 2}[order]
    return (poly * phi).to(dtype)


def _filter_axis(img, taps, dim):
    """cross-correlation of (B, C, a, b, c) with taps along spatial axis dim, zero padding"""
    B, C = img.shape[:2]
    view = [1, 1, 1, 1, 1]
    view[dim + 2] = -1
    pad = [0, 0, 0]
    pad[dim] = taps.shape[0] // 2
    return F.conv3d(img.reshape(B * C, 1, *img.shape[2:]), taps.view(view), padding=pad).reshape(img.shape)


def softmesh_field(logits, coords, res=RES, smooth_sigma=SMOOTH_SIGMA, sig=SIG, **kw):
    """SoftMesh.forward up to the PSR grid: logits (B, K, N), coords (B, 3, N) -> (B (K - 1), *res)"""
    B, K, N = logits.shape
    p = logits.softmax(1)[:, 1:]
    pts = coords.transpose(1, 2)
    seg = splat(p, pts, res, "torch").transpose(-1, -3)
    taps = derivative_taps(smooth_sigma, 1, 1.5, torch.float64).to(logits.dtype).to(logits.device)
    normals = torch.stack([_filter_axis(seg, taps, d) for d in (2, 1, 0)], 2).reshape(B * (K - 1), 3, *res)
    return psr_field(pts.repeat_interleave(K - 1, 0), normals, res, sig, **kw)


# ------------------------------------------------------------------ the bar
FLOOR = 8 * 2.0 ** -24


def bar(tag, label, got, want64, want32, magnitude=None):
    """|got - oracle64| <= max(4 |oracle32 - oracle64|, 8 * 2^-24 * magnitude) -> (ok, message); prints the measured figures"""
    want64 = want64.double().cpu()
    got, want32 = got.double().cpu(), want32.double().cpu()
    mag = float(want64.abs().max()) if magnitude is None else magnitude
    err = float((got - want64).abs().max()) if got.numel() else 0.0
    own = float((want32 - want64).abs().max()) if got.numel() else 0.0
    rel = (lambda x: x / mag) if mag > 0 else (lambda x: x)
    print(f"{tag} {label}: err {rel(err):.3e} oracle32 {rel(own):.3e} magnitude {mag:.3e}")
    return err <= max(4 * own, FLOOR * mag), f"{label}: err {err:.3e}, oracle32 {own:.3e}, magnitude {mag:.3e}"
