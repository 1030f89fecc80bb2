"""Dense Adam image registration (csrc/dense_reg.hip)."""
import torch

from .. import _lib
from .._launch import _amp_bwd, _amp_fwd, _f32c, _need_gpu, _p, launch


# ------------------------------------------------------------------ dense Adam image registration (csrc/dense_reg.hip)
def _reg_field(field, name, channels=None):
    if not torch.is_tensor(field) or not field.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, got {field.dtype if torch.is_tensor(field) else type(field).__name__}")
    if field.dim() != 5 or field.shape[0] < 1 or field.shape[1] < 1 or (channels is not None and field.shape[1] != channels):
        want = "(B, C, S0, S1, S2)" if channels is None else f"(B, {channels}, S0, S1, S2)"
        raise ValueError(f"expected {name} {want}, got {tuple(field.shape)}")
    if min(field.shape[2:]) < 3:
        raise ValueError(f"{name}: every spatial axis must be >= 3 (avg_pool3d's own limit for a kernel of 3), got "
                         f"{tuple(field.shape[2:])}")
    if field.shape[2] * field.shape[3] * field.shape[4] >= 2 ** 31 or field.shape[0] * field.shape[1] > 65535:
        raise ValueError(f"{name}: S0 S1 S2 must be < 2^31 and B C <= 65535, got {tuple(field.shape)}")


def _reg_smooth3_raw(x):
    B, C, S0, S1, S2 = x.shape
    out = torch.empty_like(x)
    launch(x.device, "fsg_reg_smooth3_f32", _p(x), B, C, S0, S1, S2, _p(out))
    return out


class _RegSmooth3(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, field):
        return _reg_smooth3_raw(_f32c(field))

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):          # the operator is its own adjoint (and linear: this backward is differentiable again)
        return _RegSmooth3.apply(g)


def reg_smooth3(field):
    """field (B, C, S0, S1, S2) -> the same shape, fp32: avg_pool3d(kernel 3, stride 1, padding 1) applied three times, the
    "B-spline" smoothing of shape_model/adam_registration.py:110-111 and :129-130, in one launch.  Zero boundary after every pool,
    so near the borders it is not the truncated [1 3 6 7 6 3 1] / 27.  Self-adjoint: the backward is the same launch on the
    incoming gradient.  Every spatial axis >= 3."""
    _reg_field(field, "field")
    _need_gpu(field)
    return _RegSmooth3.apply(field)


def reg_pack_features(feat):
    """feat (B, C, S0, S1, S2) of any floating type -> (B, S0, S1, S2, Cp) fp16, channels last, Cp = C rounded up to a multiple
    of 8, the pad channels zero: the layout reg_objective reads with 16-byte loads (pass it `channels=C`).  The reference holds
    its features in fp16 as well (adam_registration.py:90-91), so nothing is lost.  Plain torch, once per registration; works
    on CPU tensors too."""
    if not torch.is_tensor(feat) or not feat.is_floating_point() or feat.dim() != 5 or feat.shape[1] < 1:
        raise ValueError(f"expected floating-point features (B, C, S0, S1, S2), got "
                         f"{tuple(feat.shape) if torch.is_tensor(feat) else type(feat).__name__}")
    B, C, S0, S1, S2 = feat.shape
    Cp = (C + 7) // 8 * 8
    out = torch.zeros(B, S0, S1, S2, Cp, dtype=torch.float16, device=feat.device)
    out[..., :C] = feat.detach().permute(0, 2, 3, 4, 1).to(torch.float16)
    return out


def _reg_features_check(B, sizes, device, feat_fix, feat_mov, channels):
    """the packed feature volumes of a (B, 3) + sizes field on `device` -> the real channel count C"""
    for f, name in ((feat_fix, "feat_fix"), (feat_mov, "feat_mov")):
        if not torch.is_tensor(f) or f.dtype != torch.float16 or f.dim() != 5:
            raise ValueError(f"{name} must be a packed fp16 tensor (B, S0, S1, S2, Cp) (reg_pack_features), got "
                             f"{(tuple(f.shape), f.dtype) if torch.is_tensor(f) else type(f).__name__}")
        if f.shape[4] % 8 or f.shape[4] < 8 or f.shape[4] > 4096:
            raise ValueError(f"{name}: the padded channel count Cp must be a multiple of 8 in 8 .. 4096, got {f.shape[4]}")
        if tuple(f.shape[:4]) != (B,) + tuple(sizes):
            raise ValueError(f"{name} {tuple(f.shape)} does not match the field (B, 3, S0, S1, S2) = {(B, 3) + tuple(sizes)}")
        if f.device != device:
            raise ValueError(f"{name} and the field are on different devices ({f.device}, {device})")
    if feat_fix.shape != feat_mov.shape:
        raise ValueError(f"feat_fix {tuple(feat_fix.shape)} and feat_mov {tuple(feat_mov.shape)} differ")
    C = feat_fix.shape[4] if channels is None else int(channels)
    if not 1 <= C <= feat_fix.shape[4]:
        raise ValueError(f"channels must be in 1 .. Cp = {feat_fix.shape[4]}, got {channels}")
    return C


def _reg_objective_check(disp, feat_fix, feat_mov, channels):
    _reg_field(disp, "disp", 3)
    return _reg_features_check(disp.shape[0], disp.shape[2:], disp.device, feat_fix, feat_mov, channels)


def _reg_objective_raw(disp, feat_fix, feat_mov, C, lambda_weight, cost_scale, grad, loss, ws):
    """disp, grad (B, 3, S0, S1, S2) fp32 contiguous, the packed features contiguous, loss (B, 2) fp32, ws the workspace: the
    launches alone, into the caller's buffers (the registration loop owns them, so nothing is allocated per iteration)"""
    B, _, S0, S1, S2 = disp.shape
    launch(disp.device, "fsg_reg_objective_f16", _p(disp), _p(feat_fix), _p(feat_mov), B, C, feat_fix.shape[4], S0, S1, S2,
           float(lambda_weight), float(cost_scale), _p(grad), _p(loss), _p(ws), ws.numel())


class _RegObjective(torch.autograd.Function):
    # (the packed features arrive as int16 views of their fp16 bits, so that cast_inputs leaves them alone under autocast)
    @staticmethod
    @_amp_fwd
    def forward(ctx, disp, feat_fix, feat_mov, C, lambda_weight, cost_scale):
        ctx.set_materialize_grads(False)
        disp = _f32c(disp)
        B, _, S0, S1, S2 = disp.shape
        grad = torch.empty_like(disp)
        loss = torch.empty(B, 2, dtype=torch.float32, device=disp.device)
        ws = _lib.workspace("fsg_reg_objective", B, S0, S1, S2, device=disp.device)
        _reg_objective_raw(disp, feat_fix, feat_mov, C, lambda_weight, cost_scale, grad, loss, ws)
        ctx.save_for_backward(grad)
        return loss[:, 0].clone(), loss[:, 1].clone()

    @staticmethod
    @_amp_bwd
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cost, g_reg):
        # one gradient is stored, that of cost + reg: the two outputs are meant to be added (the reference's loss + reg_loss),
        # so their incoming gradients are equal, per item; the stored gradient is scaled by it
        if g_cost is None or g_reg is None:
            raise RuntimeError("reg_objective: cost and reg must both enter the loss, with the same weight (the launch forms "
                               "the gradient of cost + reg)")
        grad, = ctx.saved_tensors
        return grad * g_cost.to(torch.float32).view(-1, 1, 1, 1, 1), None, None, None, None, None


def reg_objective(disp, feat_fix, feat_mov, lambda_weight, cost_scale=12., channels=None):
    """The objective of shape_model/adam_registration.py:112-122 in one fused gather: disp (B, 3, S0, S1, S2) the smoothed field
    (channel c displaces along axis S_c), feat_fix / feat_mov packed by reg_pack_features, `channels` the real channel count C
    (default: all Cp) -> (cost (B,), reg (B,)): cost = cost_scale * mean over nodes and channels of (sample - fix)^2 with the
    moving features sampled trilinearly with zero padding at identity + disp / ((S - 1) / 2), reg = lambda_weight * the three
    means of squared forward differences.  The gradient of cost + reg with respect to disp is formed by the same launch and
    scaled in the backward: the two outputs must enter the loss with the SAME weight (as `cost + reg` does; the backward uses
    the gradient arriving at `cost`).  Gradient for disp only, no double backward.  Any disp is legal (far outside, inf, NaN
    read 0); lambda_weight == 0 skips the regulariser."""
    C = _reg_objective_check(disp, feat_fix, feat_mov, channels)
    _need_gpu(disp, feat_fix, feat_mov)
    return _RegObjective.apply(disp, feat_fix.contiguous().view(torch.int16), feat_mov.contiguous().view(torch.int16), C,
                               float(lambda_weight), float(cost_scale))
