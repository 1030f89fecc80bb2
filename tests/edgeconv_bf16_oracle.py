"""Rounded-operand model of the two-layer EdgeConv in bf16 operand mode (csrc/edgeconv2.hip: fsg_edgeconv2_{fwd,bwd}_bf16), in
plain torch, device- and dtype-agnostic; no project kernel runs here.  Pinned by tests/test_edgeconv_bf16_oracle_cpu.py, used by
tests/test_edgeconv_bf16_gpu.py.

The model starts at the per-point rows pq = [P | Q] (B,N,128) -- the first-layer Linear is tested elsewhere and must put no
noise in front of the rounding -- and restates what the kernels compute, stage by stage (rnd = round-to-nearest-even to bf16):
    y1 = P_j + Q_i;  BN1;  z1 = LeakyReLU(a1 y1 + b1);  y2 = rnd(z1) rnd(W2)^T;  BN2 statistics of THAT y2;  selection over k
    dy2 = a2 (h - db2/M - yhat2 dg2/M);  dz1 = rnd(dy2) rnd(W2);  dW2 = rnd(dy2)^T rnd(z1);  du1 = dz1 f'(u1);
    BN1's backward and the gather to grad_pq.
The backward is the KERNEL's, not autograd through the rounding: rnd has no derivative, the kernel treats it as the identity.
The selected slot and the sign of u2 there are ARGUMENTS of the backward (the GPU tests take them from the kernel), so a
re-routed arg-max moves no row out of the comparison.

In float64 the model is the oracle (rnd is exact: frexp, round-half-even, an exact power of two).  In float32, with .bfloat16().float() as
rnd, the same function is the yardstick: what any fp32 implementation of the rounded model loses against the oracle.

Rounding ambiguity.  An operand v that carries fp32 noise n(v) may legitimately round to either neighbour when it lies within
n(v) of the midpoint between two adjacent bf16 values; it then moves by one ulp, 2^(floor(log2 |v|) - 7).  For z1 the noise is
    n = C_Z 2^-24 (|a1 y1| + |beta1| + |mu1 a1|), times the slope where u1 < 0
(one rounding each of y1, a1, b1 = beta1 - mu1 a1 and the fma, at the size of the summed terms, not of the result), and
    T_flip(y2[e,o]) = sum_c amb(z1[e,c]) ulp(z1[e,c]) |rnd W2[o,c]|
is what the flips can move an output by.  C_Z = 6 as for the near-ties of edgeconv_oracle (ten times the rms fp32 error)."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import edgeconv_oracle as eo

C1 = 64
C_Z = 6.0
MAX_AMBIGUOUS = 0.01            # share of z1 operands that may be ambiguous (a condition on the inputs)
MAX_LEFT_OUT = 0.02             # share of rows on the LeakyReLU kink of layer 2 (tests/test_edgeconv_gpu.py)

# (B, N, k, C2, train, seed, fp32_mfma): the split kernels (C2 = 64), then the fp32-MFMA kernels with BF = true
CASES_SPLIT = [(2, 300, 20, 64, True, 41, False), (2, 130, 40, 64, True, 42, False), (64, 61, 20, 64, True, 43, False),
               (48, 50, 40, 64, True, 44, False), (2, 77, 25, 64, False, 45, False), (2, 100, 3, 64, True, 46, False),
               (1, 37, 1, 64, False, 47, False), (1, 90, 64, 64, True, 48, False)]
CASES_MFMA = [(2, 130, 40, 128, True, 51, False), (1, 77, 7, 128, False, 52, False), (128, 40, 20, 128, True, 53, False),
              (2, 300, 20, 64, True, 41, True)]
CASES = CASES_SPLIT + CASES_MFMA


def case_id(case):
    B, N, k, C2, train, _, dbg = case
    return "%dx%d-k%d-c%d-%s%s" % (B, N, k, C2, "train" if train else "eval", "-fp32mfma" if dbg else "")


# ------------------------------------------------------------------------------------------------------------ rounding
def _pow2(e):
    """2^e as float64, built from its bit pattern: exact on every device (a pow() may be an ulp off, and the rounded values
    must be bf16 values to the bit)"""
    return ((e.long() + 1023) << 52).view(torch.float64)


def rnd_bf16(v):
    """round to nearest even to bf16, returned in the dtype of v.  float64: exact (no detour through float32)."""
    if v.dtype != torch.float64:
        return v.bfloat16().to(v.dtype)
    m, e = torch.frexp(v)                       # |m| in [0.5, 1): eight significant bits are m * 256 rounded to an integer
    return torch.round(m * 256.0) * _pow2(e - 8)


def trunc_bf16(v):
    """the MUTANT rounding: the low sixteen bits of the fp32 pattern dropped (towards zero)"""
    if v.dtype != torch.float64:
        return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(v.dtype)
    m, e = torch.frexp(v)
    return torch.trunc(m * 256.0) * _pow2(e - 8)


def identity(v):
    return v


def bf16_ulp(v):
    """2^(floor(log2 |v|) - 7) in float64: the spacing of bf16 values in the binade of v"""
    _, e = torch.frexp(v.double())
    return _pow2(e - 8)


def midpoint_distance(v):
    """distance of v to the nearest midpoint between two adjacent bf16 values (float64)"""
    m, e = torch.frexp(v.double().abs())
    s = m * 256.0
    frac = s - torch.floor(s)
    d = (frac - 0.5).abs()
    # at the bottom of a binade the midpoint below belongs to the finer grid underneath: a quarter of this binade's ulp below 128
    d = torch.where(torch.floor(s) == 128.0, torch.minimum(d, frac + 0.25), d)
    return d * _pow2(e - 8)


# ------------------------------------------------------------------------------------------------------------ graphs, inputs
def graph_kind(N, k):
    if k == 1:
        return "self"
    return "degrees" if N * k >= sum(eo.STANDARD_DEGREES) else "random"


def make_graph(B, N, k, seed):
    kind = graph_kind(N, k)
    if kind == "degrees":
        return eo.graph_with_in_degrees(B, N, k, seed=seed)
    if kind == "self":
        return torch.arange(N, dtype=torch.int32).view(1, N, 1).expand(B, N, k).contiguous()
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    idx[:, :, 0] = np.arange(N)
    return torch.from_numpy(idx)


def case_inputs(case):
    """float32 inputs of a case: pq (B,N,128) = N(0,1) rows with a per-channel offset and scale (BatchNorm 1 has work to do),
    W2 (C2,64), (gamma, beta, running mean, running var) of both BatchNorms, the output gradient G (B,N,C2), the graph"""
    B, N, k, C2, train, seed, _ = case
    rng = np.random.default_rng(seed)
    off, sc = 0.5 * rng.standard_normal(128), 0.5 + rng.random(128)
    pq = (rng.standard_normal((B, N, 128)) * sc + off).astype(np.float32)
    bn1 = eo.layer_params(rng, 1, C1)[1:]
    W2, *bn2 = eo.layer_params(rng, C1, C2)
    G = rng.standard_normal((B, N, C2)).astype(np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    return SimpleNamespace(case=case, B=B, N=N, k=k, C2=C2, train=train, pq=T(pq), W2=T(W2), bn1=[T(a) for a in bn1],
                           bn2=[T(a) for a in bn2], G=T(G), idx=make_graph(B, N, k, seed))


# ------------------------------------------------------------------------------------------------------------ the model
def _bn_stats(y, rm, rv, train, eps, momentum):
    M = y.shape[0] * y.shape[1] * y.shape[2]
    if train:
        mu, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
        rm = (1 - momentum) * rm + momentum * mu
        rv = (1 - momentum) * rv + momentum * var * (M / max(M - 1, 1))
    else:
        mu, var = rm, rv
    return mu, 1.0 / torch.sqrt(var + eps), rm, rv


def forward(pq, idx, W2, bn1, bn2, train, slope=0.2, eps=1e-5, momentum=0.1, rz=rnd_bf16, rw=rnd_bf16):
    """The forward of the rounded model in the dtype of pq.  bn1 / bn2 = (gamma, beta, running mean, running var).  rz / rw: the
    rounding of z1 / W2 (identity switches it off, trunc_bf16 is a mutant).  Returns everything the backward and the judges
    need: y1, u1, z1, zr = rz(z1), Wr, y2 (B,N,k,C2), mag = |zr| |Wr|^T, mu / r (mean, 1/std) and the new running statistics of
    both layers, the model's own selection slot (B,N,C2) with ysel, u2sel, out_pm (B,N,C2)."""
    B, N, _ = pq.shape
    k = idx.shape[2]
    g1, b1, rm1, rv1 = bn1
    g2, b2, rm2, rv2 = bn2
    flat = (idx.long().to(pq.device) + torch.arange(B, device=pq.device).view(B, 1, 1) * N).reshape(-1)
    y1 = pq[..., :C1].reshape(B * N, C1)[flat].view(B, N, k, C1) + pq[..., C1:].unsqueeze(2)
    mu1, r1, rm1n, rv1n = _bn_stats(y1, rm1, rv1, train, eps, momentum)
    u1 = (y1 - mu1) * r1 * g1 + b1
    z1 = F.leaky_relu(u1, slope)
    zr, Wr = rz(z1), rw(W2)
    y2 = zr @ Wr.t()
    mu2, r2, rm2n, rv2n = _bn_stats(y2, rm2, rv2, train, eps, momentum)
    sgn = torch.where(g2 >= 0, torch.ones_like(g2), -torch.ones_like(g2))
    slot = (y2 * sgn).argmax(2)
    ysel = torch.gather(y2, 2, slot.unsqueeze(2)).squeeze(2)
    u2sel = (ysel - mu2) * r2 * g2 + b2
    return SimpleNamespace(B=B, N=N, k=k, flat=flat, train=train, slope=slope, y1=y1, u1=u1, z1=z1, zr=zr, Wr=Wr, y2=y2,
                           mag=zr.abs() @ Wr.abs().t(), mu1=mu1, r1=r1, rm1=rm1n, rv1=rv1n, mu2=mu2, r2=r2, rm2=rm2n, rv2=rv2n,
                           g1=g1, b1=b1, g2=g2, b2=b2, sgn=sgn, slot=slot, ysel=ysel, u2sel=u2sel, out_pm=F.leaky_relu(u2sel, slope))


def backward(f, G, slot=None, pos=None, rd=rnd_bf16):
    """The kernel's backward on a forward() result: G (B,N,C2) gradient of the point-major output, slot (B,N,C2) the selected
    edge and pos (B,N,C2, bool) whether u2 > 0 there (default: the model's own).  rd: the rounding of dy2.
    -> dict(pq (B,N,128), W2, gamma1, beta1, gamma2, beta2) and the intermediates dr = rd(dy2), dy1 (B,N,k,64), h."""
    B, N, k = f.B, f.N, f.k
    M = B * N * k
    slot = f.slot if slot is None else slot.long()
    pos = (f.u2sel > 0) if pos is None else pos
    one = torch.ones_like(G)
    h = G * torch.where(pos, one, f.slope * one)
    ysel = torch.gather(f.y2, 2, slot.unsqueeze(2)).squeeze(2)
    db2, dg2 = h.sum((0, 1)), (h * (ysel - f.mu2) * f.r2).sum((0, 1))
    dy2 = torch.zeros_like(f.y2).scatter_(2, slot.unsqueeze(2), h.unsqueeze(2))
    if f.train:
        dy2 = dy2 - db2 / M - (f.y2 - f.mu2) * f.r2 * (dg2 / M)
    dr = rd(dy2 * (f.g2 * f.r2))
    dz1 = dr @ f.Wr
    dW2 = dr.reshape(M, -1).t() @ f.zr.reshape(M, C1)
    du1 = dz1 * torch.where(f.u1 > 0, torch.ones_like(dz1), f.slope * torch.ones_like(dz1))
    yhat1 = (f.y1 - f.mu1) * f.r1
    db1, dg1 = du1.sum((0, 1, 2)), (du1 * yhat1).sum((0, 1, 2))
    dy1 = du1
    if f.train:
        dy1 = du1 - db1 / M - yhat1 * (dg1 / M)
    dy1 = dy1 * (f.g1 * f.r1)
    gP = torch.zeros(B * N, C1, dtype=dy1.dtype, device=dy1.device).index_add_(0, f.flat, dy1.reshape(M, C1))
    return dict(pq=torch.cat([gP.view(B, N, C1), dy1.sum(2)], -1), W2=dW2, gamma1=dg1, beta1=db1, gamma2=dg2, beta2=db2,
                dr=dr, dy1=dy1, h=h)


GRADS = ("W2", "gamma1", "beta1", "gamma2", "beta2")


def run(inp, dtype, device="cpu", slot=None, pos=None, rz=rnd_bf16, rw=rnd_bf16, rd=rnd_bf16):
    """forward + backward of a case's inputs in `dtype` on `device` -> (forward namespace, gradient dict)"""
    c = lambda t: t.to(device=device, dtype=dtype)   # noqa: E731
    with torch.no_grad():
        f = forward(c(inp.pq), inp.idx.to(device), c(inp.W2), [c(t) for t in inp.bn1], [c(t) for t in inp.bn2], inp.train, rz=rz, rw=rw)
        g = backward(f, c(inp.G), slot, pos, rd)
    return f, g


# ------------------------------------------------------------------------------------------------------------ ambiguity
def z1_noise(f, c_z=C_Z):
    """fp32 noise of z1 (float64, shape of z1), see the module docstring; f: a float64 forward()"""
    a1 = (f.g1 * f.r1).double()
    n = c_z * 2.0 ** -24 * ((a1 * f.y1.double()).abs() + f.b1.double().abs() + (f.mu1.double() * a1).abs())
    return torch.where(f.u1 < 0, f.slope * n, n)


def ambiguous(f, c_z=C_Z):
    """bool, shape of z1: the operands whose bf16 rounding an fp32 implementation may legitimately take the other way"""
    return midpoint_distance(f.z1) <= z1_noise(f, c_z)


def t_flip(f, amb):
    """(B,N,k,C2) float64: what the ambiguous operands can move y2 by"""
    return (amb.double() * bf16_ulp(f.z1)) @ f.Wr.double().abs().t()


def kink_rows(f, bound):
    """rows (B*N, bool) with a channel whose u2 at the selected slot lies within |a2| x its bound (B,N,C2) of the LeakyReLU kink"""
    return ((f.u2sel.abs() <= (f.g2 * f.r2).abs() * bound).any(-1)).reshape(-1)


def row_errors(got, want):
    """the per-row figures that edgeconv_oracle.row_error takes the maximum of: |got_r - want_r| / (|want_r| + rms row norm)"""
    want = want.double().reshape(-1, want.shape[-1])
    rn = want.norm(dim=1)
    return (got.double().reshape(want.shape) - want).norm(dim=1) / (rn + rn.pow(2).mean().sqrt())


def at_slot(t, slot):
    return torch.gather(t, 2, slot.long().unsqueeze(2)).squeeze(2)


# ------------------------------------------------------------------------------------------------------------ tiling mirror
SPLIT_WG_FWD, SPLIT_WG_BWD = 768, 512          # workgroups of the split kernels over the B clouds
MFMA_WG_FWD, MFMA_WG_BWD = 1024, 768           # ... of the fp32-MFMA kernels
TP_MAX = 16                                    # a tile's Q rows are staged with one 16-byte piece per thread
RT_GAIN = 1.15                                 # 128-row tiles when they cut the padding by more than 15 %


def ec2s_tiling(k, B, N, bwd, bf16):
    """(RT, TP, G) of the split kernels, as csrc/edgeconv2.hip ec2s_tiling.  u2 / u4 in float32 like the C code."""
    tp2, tp4 = 64 // k, 128 // k
    u2, u4 = np.float32(tp2 * k) / np.float32(64), np.float32(tp4 * k) / np.float32(128)
    RT = 4 if u4 > np.float32(RT_GAIN) * u2 else 2
    if not bwd and not bf16:
        RT = 2
    TP = min(max(tp4 if RT == 4 else tp2, 1), TP_MAX)
    ntiles = (N + TP - 1) // TP
    G = min(max((SPLIT_WG_BWD if bwd else SPLIT_WG_FWD) // B, 1), ntiles)
    return RT, TP, G


def ec2_tiling(k, B, N, bwd):
    """(TP, Rpad, G) of the fp32-MFMA kernels (ec2_tiling / ec2_bwd_tiling)"""
    TP = max(64 // k, 1)
    Rpad = (TP * k + 31) & ~31
    ntiles = (N + TP - 1) // TP
    G = min(max((MFMA_WG_BWD if bwd else MFMA_WG_FWD) // B, 1), ntiles)
    return TP, Rpad, G
