"""Torch restatement, on the CPU, of the dense Adam registration loop (reference: shape_model/adam_registration.py:93-132), written
for this repository: the triple zero-padded pool, the objective under autograd, the Adam loop and the upsampling.  Run in fp64
it is the reference of tests/test_dense_reg_*.py, run in fp32 it is the yardstick: a kernel may miss the fp64 result by at most
4 x what this composition misses it by in fp32 on the same input, with a floor of 8 * 2^-24 = 4.8e-7, errors relative to the
largest magnitude of the quantity (`bar`).  Measured pairs are printed and, when FSG_REG_PARITY names a file, appended to it."""
import os

import torch
from torch.nn import functional as F

FLOOR = 8 * 2.0 ** -24
GRID_SP = 2


def smooth3(x):
    """avg_pool3d(kernel 3, stride 1, padding 1) three times (count_include_pad=True is the default)"""
    for _ in range(3):
        x = F.avg_pool3d(x, 3, stride=1, padding=1)
    return x


def truncated7(x):
    """what the triple pool is NOT at the borders: the 7-tap [1 3 6 7 6 3 1] / 27 per axis over a zero-padded input"""
    B, C = x.shape[:2]
    k = torch.tensor([1., 3., 6., 7., 6., 3., 1.], dtype=x.dtype) / 27
    y = x.reshape(B * C, 1, *x.shape[2:])
    y = F.conv3d(y, k.view(1, 1, 7, 1, 1), padding=(3, 0, 0))
    y = F.conv3d(y, k.view(1, 1, 1, 7, 1), padding=(0, 3, 0))
    y = F.conv3d(y, k.view(1, 1, 1, 1, 7), padding=(0, 0, 3))
    return y.reshape(x.shape)


def regulariser(disp, lam):
    """:112-114 per item: lam * the mean squared forward difference along each spatial axis; lam == 0 -> 0 (not evaluated)"""
    if lam == 0:
        return disp.new_zeros(disp.shape[0])
    d = disp.permute(0, 2, 3, 4, 1)
    return lam * ((d[:, :, 1:] - d[:, :, :-1]) ** 2).mean((1, 2, 3, 4)) + \
        lam * ((d[:, 1:] - d[:, :-1]) ** 2).mean((1, 2, 3, 4)) + \
        lam * ((d[:, :, :, 1:] - d[:, :, :, :-1]) ** 2).mean((1, 2, 3, 4))


def objective(disp, feat_fix, feat_mov, lam, cost_scale=12., zero_nodes=None):
    """:112-122.  disp (B, 3, S0, S1, S2) the smoothed field, features (B, C, S0, S1, S2), all of one dtype -> (cost (B,),
    reg (B,)).  zero_nodes (B, S0, S1, S2) bool: nodes whose sample is defined to be 0 (a coordinate that is not finite or
    absurdly far out) -- their displacement is replaced by 0 before sampling and the sample is zeroed."""
    B, _, S0, S1, S2 = disp.shape
    dt = disp.dtype
    reg = regulariser(disp, lam)
    d = disp if zero_nodes is None else torch.where(zero_nodes.unsqueeze(1), torch.zeros((), dtype=dt), disp)
    id_grid = F.affine_grid(torch.eye(3, 4, dtype=dt).unsqueeze(0).expand(B, 3, 4), (B, 1, S0, S1, S2), align_corners=False)
    scale = torch.tensor([(S0 - 1) / 2, (S1 - 1) / 2, (S2 - 1) / 2], dtype=dt)
    grid = id_grid + (d.permute(0, 2, 3, 4, 1) / scale).flip(-1)
    sampled = F.grid_sample(feat_mov, grid, align_corners=False, mode='bilinear')
    if zero_nodes is not None:
        sampled = sampled * (~zero_nodes).unsqueeze(1).to(dt)
    cost = ((sampled - feat_fix).pow(2).mean(1) * cost_scale).mean((1, 2, 3))
    return cost, reg


def objective_with_grad(disp, feat_fix, feat_mov, lam, dtype, cost_scale=12., zero_nodes=None):
    """-> cost (B,), reg (B,), d (cost + reg) / d disp, all in `dtype`"""
    d = disp.detach().to(dtype).clone().requires_grad_(True)
    cost, reg = objective(d, feat_fix.to(dtype), feat_mov.to(dtype), lam, cost_scale, zero_nodes)
    g, = torch.autograd.grad((cost + reg).sum(), d)
    return cost.detach(), reg.detach(), g


def sample_coords(disp):
    """the unnormalised sample coordinate of every node in fp64, (B, 3, S0, S1, S2): t_c = i_c + disp_c S_c / (S_c - 1)"""
    B, _, S0, S1, S2 = disp.shape
    d = disp.double()
    idx = torch.stack(torch.meshgrid(*(torch.arange(s, dtype=torch.float64) for s in (S0, S1, S2)), indexing="ij"))
    unit = torch.tensor([S0 / (S0 - 1), S1 / (S1 - 1), S2 / (S2 - 1)], dtype=torch.float64).view(1, 3, 1, 1, 1)
    return idx.unsqueeze(0) + d * unit


def near_integer(disp, eps=1e-3):
    """(B, S0, S1, S2) bool: the node's sample coordinate lies within eps of an integer on some axis, where the trilinear
    gradient is discontinuous"""
    t = sample_coords(disp)
    return ((t - t.round()).abs() < eps).any(1)


def adam_loop(feat_fix, feat_mov, iters=50, lam=.65, lr=1., cost_scale=12., perturb_ulp=False, param0=None):
    """:93-126 with torch.optim.Adam, in the dtype and on the device of the features (B, C, Hg, Wg, Dg) -> (fitted_grid,
    history (iters, B, 2)).  The parameter starts at the identity grid coordinates; perturb_ulp moves every entry of the start
    one unit in the last place up."""
    B, _, Hg, Wg, Dg = feat_fix.shape
    dt, dev = feat_fix.dtype, feat_fix.device
    id_grid = F.affine_grid(torch.eye(3, 4, dtype=dt, device=dev).unsqueeze(0).expand(B, 3, 4), (B, 1, Hg, Wg, Dg),
                            align_corners=False)
    p0 = id_grid.permute(0, 4, 1, 2, 3).contiguous() if param0 is None else param0.to(device=dev, dtype=dt).clone()
    if perturb_ulp:
        p0 = torch.nextafter(p0, torch.full_like(p0, float("inf")))
    param = torch.nn.Parameter(p0)
    opt = torch.optim.Adam([param], lr=lr)
    scale = torch.tensor([(Hg - 1) / 2, (Wg - 1) / 2, (Dg - 1) / 2], dtype=dt, device=dev)
    history = []
    for _ in range(iters):
        opt.zero_grad()
        disp = smooth3(param)
        d = disp.permute(0, 2, 3, 4, 1)
        reg = lam * ((d[:, :, 1:] - d[:, :, :-1]) ** 2).mean((1, 2, 3, 4)) + lam * ((d[:, 1:] - d[:, :-1]) ** 2).mean((1, 2, 3, 4)) + \
            lam * ((d[:, :, :, 1:] - d[:, :, :, :-1]) ** 2).mean((1, 2, 3, 4))
        grid = id_grid + (d / scale).flip(-1)
        sampled = F.grid_sample(feat_mov, grid, align_corners=False, mode='bilinear')
        cost = ((sampled - feat_fix).pow(2).mean(1) * cost_scale).mean((1, 2, 3))
        (cost + reg).sum().backward()
        history.append(torch.stack([cost.detach(), reg.detach()], 1))
        opt.step()
    return disp.detach(), torch.stack(history)


def upsample(fitted_grid, shape):
    """:127-132: x GRID_SP, trilinear upsample, triple pool, / (S - 1) * 2, channel flip"""
    hr = F.interpolate(fitted_grid * GRID_SP, size=shape, mode='trilinear', align_corners=False)
    sm = smooth3(hr)
    scale = torch.tensor([s - 1 for s in shape], dtype=fitted_grid.dtype, device=fitted_grid.device).view(1, 3, 1, 1, 1)
    return torch.flip(sm / scale * 2, [1])


def half_features(shape, seed, one_hot=False):
    """(B, C, S0, S1, S2) features as the kernel sees them: uniform in [0, 1) rounded to fp16 (or one-hot 0 / 1 channels), held
    in fp64 -- exact in every dtype the tests use"""
    g = torch.Generator().manual_seed(seed)
    B, C = shape[:2]
    if one_hot:
        lab = torch.randint(0, C, (B,) + tuple(shape[2:]), generator=g)
        return F.one_hot(lab, C).permute(0, 4, 1, 2, 3).double()
    return torch.rand(*shape, generator=g).half().double()


def blob_features(shape, seed):
    """smooth random blobs in [0, 1], (B, C, S0, S1, S2) fp64 (rounded to fp16)"""
    g = torch.Generator().manual_seed(seed)
    x = smooth3(smooth3(torch.rand(*shape, generator=g, dtype=torch.float64)))
    lo, hi = x.amin((2, 3, 4), keepdim=True), x.amax((2, 3, 4), keepdim=True)
    return ((x - lo) / (hi - lo)).half().double()


def smooth_field(sizes, seed, amplitude):
    """(1, 3, S0, S1, S2) fp64, smooth, largest entry = amplitude (in voxels)"""
    g = torch.Generator().manual_seed(seed)
    f = smooth3(smooth3(torch.randn(1, 3, *sizes, generator=g, dtype=torch.float64)))
    return f / f.abs().max() * amplitude


def warp_voxels(vol, field):
    """vol (B, C, S0, S1, S2) read at node + field (channel c along axis c, in voxels), trilinear, zero padding"""
    B, _, S0, S1, S2 = vol.shape
    dt = vol.dtype
    id_grid = F.affine_grid(torch.eye(3, 4, dtype=dt).unsqueeze(0).expand(B, 3, 4), (B, 1, S0, S1, S2), align_corners=False)
    scale = torch.tensor([S0 / 2, S1 / 2, S2 / 2], dtype=dt)
    return F.grid_sample(vol, id_grid + (field.to(dt).permute(0, 2, 3, 4, 1) / scale).flip(-1), align_corners=False)


def record(line):
    print(line)
    path = os.environ.get("FSG_REG_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def bar(label, got, want64, want32, keep=None, magnitude=None):
    """|got - oracle64| <= max(4 |oracle32 - oracle64|, FLOOR * magnitude) over the entries `keep` (default all); the magnitude
    is the largest |oracle64| over ALL entries -> (ok, message); records the measured pair"""
    want64 = want64.double().cpu()
    got, want32 = got.double().cpu(), want32.double().cpu()
    mag = float(want64.abs().max()) if magnitude is None else float(magnitude)
    e, o = (got - want64).abs(), (want32 - want64).abs()
    if keep is not None:
        e, o = e[keep], o[keep]
    err = float(e.max()) if e.numel() else 0.0
    own = float(o.max()) if o.numel() else 0.0
    rel = (lambda x: x / mag) if mag > 0 else (lambda x: x)
    record(f"REG_PARITY {label}: err {rel(err):.3e} oracle32 {rel(own):.3e} magnitude {mag:.3e}")
    return err <= max(4 * own, FLOOR * mag), f"{label}: err {err:.3e}, oracle32 {own:.3e}, magnitude {mag:.3e}"
