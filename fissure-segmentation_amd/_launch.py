"""Launch plumbing shared by `functional`, the ops modules and the other host files: the GPU-only check, pointer and stream
arguments, the autocast exits and `launch`, the one way from a tensor-level wrapper into the C ABI."""
import contextlib as _contextlib
import ctypes

import torch

from . import _lib


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fissure_segmentation_amd runs on the GPU only (got a CPU tensor); "
                               "the CPU restatement lives in oracle/ and is test infrastructure")


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------ mixed precision (model_trainer.py:75-76,157,189-193)
# The reference runs every segmentation step under `autocast` (fp16) + GradScaler.  The HIP kernels take fp32 rows and
# the graph is always built in fp32 (indices equal the fp32 CPU path), so every autograd.Function leaves the autocast
# region: floating-point inputs are cast to fp32 on entry, forward and backward run with autocast off, outputs and
# gradients are fp32.  Reduced precision is an explicit choice here (`set_mfma_operands("bf16")`), not an ambient one.
def _amp_fwd(fn):
    return torch.amp.custom_fwd(fn, device_type="cuda", cast_inputs=torch.float32)


def _amp_bwd(fn):
    return torch.amp.custom_bwd(fn, device_type="cuda")


def no_autocast():
    """context: autocast off (entered only when it is on, so CPU-only hosts see no device warning)"""
    if torch.is_autocast_enabled("cuda"):
        return torch.autocast("cuda", enabled=False)
    return _contextlib.nullcontext()


def launch(device, name, *args):
    """enter `device`, call the entry point with torch's current stream of that device appended"""
    with torch.cuda.device(device):
        _lib.call(name, *args, _stream())
