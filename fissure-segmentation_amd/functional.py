"""Tensor-level entry points over the C ABI: argument checking, output allocation, stream/device
plumbing and the autograd glue.  Every function requires CUDA (HIP) tensors -- no CPU path."""
import contextlib as _contextlib
import ctypes
import os as _os

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


# bf16 OPERAND MODE (BASELINE configs 3-5 name bf16 as their compute type).  What it changes: the operands of the dense
# contractions -- the per-edge 64 x C2 product of the two-layer EdgeConv (fsg_edgeconv2_{fwd,bwd}_bf16 on
# v_mfma_f32_32x32x16_bf16) and, with `set_bf16_linear(True)`, the Linear layers' products on the hand-written GEMMs -- are
# rounded to bf16, accumulation stays fp32.  The products that go to the vendor library stay fp32: with bf16 operands every
# call pays a cast pass over its fp32 activations and gradients, and the config-4 step was measured SLOWER on MI355X (4.64 vs
# 4.17 ms); the hand-written kernels convert their operands on the way out of LDS at no extra traffic.
# What the mode never changes: the graph build (always fp32: indices equal the fp32 CPU path), BatchNorm
# statistics, selection, every stored activation and every gradient tensor (fp32).  Switched on explicitly
# (`set_mfma_operands("bf16")` / `with mfma_operands("bf16")`) or by an ambient `torch.autocast("cuda", torch.bfloat16)`
# around a model forward; the backward of every op follows the mode its forward ran in.
_mfma_mode = "f32"


def set_mfma_operands(kind):
    global _mfma_mode
    if kind not in ("f32", "bf16"):
        raise ValueError("MFMA operand type must be 'f32' or 'bf16'")
    _mfma_mode = kind


@_contextlib.contextmanager
def mfma_operands(kind):
    global _mfma_mode
    old = _mfma_mode
    set_mfma_operands(kind)
    try:
        yield
    finally:
        _mfma_mode = old


def bf16_operands():
    return _mfma_mode == "bf16"


def _ambient_bf16():
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


_deterministic = bool(_os.environ.get("FSG_DETERMINISTIC"))


def set_deterministic(flag=True):
    """Reproducible (ordered) reductions where the default scatters with fp32 atomics: today the Chamfer backward, whose
    ordered form walks the reverse graph of the arg-min and is slow when many points share one nearest neighbour (a
    collapsed reconstruction early in training: 5.3 -> 6.3 ms per PC-AE step).  Also on under
    `torch.use_deterministic_algorithms(True)` and FSG_DETERMINISTIC=1.  The DGCNN path is reproducible regardless.
    Limit: the reverse-graph builder keeps one counter per target in LDS and takes at most 16384 targets per cloud; a Chamfer
    backward onto more targets than that uses the atomics even with the flag set (same values to fp32 rounding, not the same
    bits from run to run; tests/test_loss_family_gpu.py, case 300 -> 16400)."""
    global _deterministic
    _deterministic = bool(flag)


def deterministic():
    return _deterministic or torch.are_deterministic_algorithms_enabled()


# ------------------------------------------------------------------ dense kNN (utils/general_utils.py:315)
def knn_graph(x, k, c_knn=None, fix_diag=True, drop_first=False, return_dist=False, force_rows_kernel=False,
              _debug_flags=0, out=None, prepared=None, pq_weight=None):
    """x: (B,C,N) -> idx (B,N,k) int32 [, dist (B,N,k) fp32].  Channel slices are passed by stride.  `out`: a contiguous
    (B,N,k) int32 tensor to write the graph into (e.g. a slice of one buffer holding all graphs of a step, so that their
    reverse graphs can be built in one launch: build_reverse_graphs).  `prepared` = (workspace, x_pm): the producer of x has
    already emitted the build's prep products into `workspace` (edgeconv1 / edgeconv2 with knn_ws=) and x_pm is its point-major
    copy (B,N,C): the build starts at its main kernel (include/fsg_hip.h: fsg_knn_dense_prepared_f32).
    `pq_weight` (rows, C) with C = c_knn <= 4 (the [W_rel ; W_ctr - W_rel] weight of the FIRST EdgeConv's first conv): the build
    also emits that block's per-point rows pq (B, N, rows) = x^T pq_weight^T (fsg_knn_dense_ws_pq_f32) -> returns (idx, pq); pq is
    None when the shape does not qualify (then the caller runs the product itself).
    `_debug_flags`: _lib.KNN_DBG_* bits, and _lib.KNN_FORCE_MFMA for the first MFMA design of libfsg_hip_experiments.so (an
    independent cross-check for tests / tools)."""
    _need_gpu(x)
    if x.dim() != 3:
        raise ValueError(f"expected (B,C,N), got {tuple(x.shape)}")
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()  # the graph is always built in fp32 (precision)
    if x.stride(2) != 1:
        x = x.contiguous()
    B, C, N = x.shape
    c_knn = C if c_knn is None else c_knn
    if out is not None:
        if out.shape != (B, N, k) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != x.device:
            raise ValueError("knn_graph: `out` must be a contiguous (B,N,k) int32 tensor on the input's device")
        idx = out
    else:
        idx = torch.empty(B, N, k, dtype=torch.int32, device=x.device)
    dist = torch.empty(B, N, k, dtype=torch.float32, device=x.device) if return_dist else None
    flags = (_lib.KNN_FIX_DIAG if fix_diag else 0) | (_lib.KNN_DROP_FIRST if drop_first else 0) | \
        (_lib.KNN_FORCE_ROWS if force_rows_kernel else 0) | _debug_flags
    if prepared is not None and c_knn == C and not return_dist and not force_rows_kernel and not _debug_flags:
        ws, x_pm = prepared
        with torch.cuda.device(x.device):
            _lib.call("fsg_knn_dense_prepared_f32", _p(x_pm), B, N, C, k, flags, _p(idx), None, _p(ws), ws.numel() * ws.element_size(),
                      _stream())
        return idx
    xx = _lib.workspace("fsg_knn_dense", B, N, c_knn, device=x.device)
    ws_bytes = xx.numel() if xx is not None else 0
    if pq_weight is not None:
        rows = pq_weight.shape[0]
        if (C == c_knn and c_knn <= 4 and tuple(pq_weight.shape) == (rows, C) and 256 % rows == 0 and not return_dist and
                not (_debug_flags & _lib.KNN_FORCE_MFMA)):
            pq = torch.empty(B, N, rows, dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _lib.call("fsg_knn_dense_ws_pq_f32", _p(x), B, N, x.stride(0), x.stride(1), c_knn, k, flags, _p(idx), None, _p(xx),
                          ws_bytes, _p(_f32c(pq_weight.detach())), rows, _p(pq), _stream())
            return idx, pq
    with torch.cuda.device(x.device):
        rc = 3   # FSG_ERR_UNSUPPORTED (also: a shape outside the experimental kernel's envelope) -> the production kernel
        if flags & _lib.KNN_FORCE_MFMA:
            xl = _lib.experiments()
            rc = xl.fsg_knn_experiment_f32(_p(x), B, N, x.stride(0), x.stride(1), c_knn, k, flags, _p(idx), _p(dist), _p(xx),
                                           _stream())
            if rc not in (0, 3):
                raise RuntimeError(xl.fsg_last_error().decode())
        if rc == 3:
            _lib.call("fsg_knn_dense_ws_f32", _p(x), B, N, x.stride(0), x.stride(1), c_knn, k, flags & ~_lib.KNN_FORCE_MFMA, _p(idx),
                      _p(dist), _p(xx), ws_bytes, _stream())
    if pq_weight is not None:
        return idx, None
    return (idx, dist) if return_dist else idx


# ------------------------------------------------------------------ edge features (models/dgcnn.py:31-36)
class _EdgeGather(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, idx):
        B, C, N = x.shape
        k = idx.shape[2]
        half = x.dtype == torch.bfloat16       # bf16 storage: fsg_edge_gather_*_bf16
        xc = x.detach().contiguous() if half else _f32c(x)
        out = torch.empty(B, 2 * C, N, k, dtype=xc.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("fsg_edge_gather_fwd_bf16" if half else "fsg_edge_gather_fwd_f32", _p(xc), _p(idx), _p(out), B, C, N, k,
                      _stream())
        ctx.save_for_backward(idx)
        ctx.shape = (B, C, N, k)
        ctx.half = half
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, C, N, k = ctx.shape
        half = ctx.half and g.dtype == torch.bfloat16
        g = g.detach().contiguous() if half else _f32c(g)
        gx = torch.empty(B, C, N, dtype=torch.float32, device=g.device)      # accumulated in fp32 in both modes
        with torch.cuda.device(g.device):
            _lib.call("fsg_edge_gather_bwd_bf16" if half else "fsg_edge_gather_bwd_f32", _p(g), _p(idx), _p(gx), B, C, N, k,
                      _stream())
        return (gx.to(torch.bfloat16) if ctx.half else gx), None


def knn_edge_features(x, k, knn_only_over_coords=False):
    """create_neighbor_features (models/dgcnn.py:15-36) with a dynamic graph, one C-ABI call: x (B,C,N) fp32 ->
    (edge (B,2C,N,k), idx (B,N,k) int32).  Forward only (the differentiable composition is knn_graph + edge_features)."""
    _need_gpu(x)
    xc = _f32c(x)
    B, C, N = xc.shape
    idx = torch.empty(B, N, k, dtype=torch.int32, device=x.device)
    edge = torch.empty(B, 2 * C, N, k, dtype=torch.float32, device=x.device)
    c_knn = 3 if knn_only_over_coords else C
    ws = _lib.workspace("fsg_knn_dense", B, N, c_knn, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("fsg_knn_gather_fused_ws_f32", _p(xc), B, C, N, k, c_knn, _p(idx), _p(edge), _p(ws), ws.numel(), _stream())
    return edge, idx


def edge_features(x, idx):
    """x (B,C,N) fp32, idx (B,N,k) int32/int64 -> (B,2C,N,k) = cat(x_j - x_i, x_i)."""
    _need_gpu(x, idx)
    if idx.dtype != torch.int32:
        idx = idx.to(torch.int32)
    return _EdgeGather.apply(x, idx.contiguous())


# ------------------------------------------------------------------ point-major linear layer (1x1 conv as one GEMM)
SMALL_GEMM_FLOPS = 6e8   # below this the vendor GEMM tends to pick one huge macro-tile (one workgroup): use fsg_gemm_small_f32


def gemm_small(a, sa_i, sa_k, b, sb_k, sb_j, bias, I, J, K, rowsum=False, defer=False, bf16=False):
    """C (I,J) = A(i,k) B(k,j) (+ bias[j]) with explicit element strides -- include/fsg_hip.h: fsg_gemm_small_f32.
    rowsum=True: also sum_k A(i,k) (fsg_gemm_small_rowsum_f32: the bias gradient next to a weight gradient) -> (C, rowsum).
    defer=True (no bias): the split reduction is left to ONE launch for all deferred products of the running backward pass
    (fsg_gemm_small_reduce_many_f32 from an end-of-backward callback of the autograd engine; at once outside a backward pass):
    the returned tensors are complete when `loss.backward()` returns -- for weight gradients, which nothing reads before.
    bf16=True: operands rounded to bf16 inside the kernel, bf16 matrix instruction, fp32 accumulation (fsg_gemm_small_bf16)."""
    out = torch.empty(I, J, dtype=torch.float32, device=a.device)
    ws = _lib.workspace("fsg_gemm_small", I, J, K, device=a.device)
    rs = torch.empty(I, dtype=torch.float32, device=a.device) if rowsum else None
    with torch.cuda.device(a.device):
        if defer and bias is None:
            splits = ctypes.c_int(0)
            if bf16:
                _lib.call("fsg_gemm_small_bf16", _p(a), sa_i, sa_k, _p(b), sb_k, sb_j, None, _p(out), J, I, J, K, _p(rs), _p(ws),
                          ctypes.byref(splits), _stream())
            else:
                _lib.call("fsg_gemm_small_deferred_f32", _p(a), sa_i, sa_k, _p(b), sb_k, sb_j, _p(out), J, I, J, K, _p(rs), _p(ws),
                          ctypes.byref(splits), _stream())
            if splits.value > 1:
                # raw addresses, not the tensors: AccumulateGrad takes a gradient over as `.grad` only when nobody else holds it
                # (it would copy -- the unreduced bytes -- otherwise); `.grad` then keeps the memory alive past the flush
                _defer_reduce((ws, out.data_ptr(), rs.data_ptr() if rs is not None else None, splits.value, I, J, a.device))
        elif bf16:
            _lib.call("fsg_gemm_small_bf16", _p(a), sa_i, sa_k, _p(b), sb_k, sb_j, _p(bias), _p(out), J, I, J, K, _p(rs), _p(ws), None,
                      _stream())
        else:
            _lib.call("fsg_gemm_small_rowsum_f32", _p(a), sa_i, sa_k, _p(b), sb_k, sb_j, _p(bias), _p(out), J, I, J, K, _p(rs),
                      _p(ws), _stream())
    return (out, rs) if rowsum else out


_pending_reduces = []     # (partials, &C, &rowsum | None, S, I, J, device) of the running backward pass
_defer_weight_grads = True


def set_deferred_weight_grads(flag):
    """Weight gradients of the small Linears that go straight to a leaf parameter are summed over their reduction splits by ONE
    launch at the end of the backward pass (default on).  Turn off when something reads parameter gradients DURING the backward
    pass (gradient hooks that copy them, e.g. torch's DistributedDataParallel buckets); this package's own
    BucketedGradAverager flushes before it reads."""
    global _defer_weight_grads
    _defer_weight_grads = bool(flag)


def _grad_targets(w):
    """the leaf parameters that the gradient of `w` ends in WITHOUT being read on the way, or None: `w` itself when it is a leaf;
    the parameters a producer names in `w._fsg_grad_unread` when its backward only hands views of the gradient on (_PackQKV)"""
    if w.is_leaf:
        return (w,)
    return getattr(w, "_fsg_grad_unread", None)


def _may_defer(targets):
    """Deferring a weight gradient's split sum to the end of the backward pass is sound when the autograd engine merely STORES the
    tensor until then: it goes to parameters whose `.grad` is empty (AccumulateGrad adopts the tensor; with a gradient already
    there it would add -- unreduced bytes), outside create_graph, and the switch is on."""
    return (_defer_weight_grads and targets is not None and not torch.is_grad_enabled() and
            all(p.grad is None for p in targets))


def flush_deferred_reduces():
    """sum the split partials of every deferred gemm_small product (see gemm_small(defer=True)); idempotent"""
    global _pending_reduces
    jobs, _pending_reduces = _pending_reduces, []
    for i0 in range(0, len(jobs), _lib.GEMM_REDUCE_MAX_JOBS):
        chunk = jobs[i0:i0 + _lib.GEMM_REDUCE_MAX_JOBS]
        tab = _lib.GemmReduceJobs()
        for i, (ws, out, rs, S, I, J, _dev) in enumerate(chunk):
            tab.part[i], tab.C[i], tab.rowsum[i] = ws.data_ptr(), out, rs
            tab.ldc[i], tab.S[i], tab.I[i], tab.J[i] = J, S, I, J
        tab.n = len(chunk)
        with torch.cuda.device(chunk[0][6]):
            _lib.call("fsg_gemm_small_reduce_many_f32", ctypes.byref(tab), _stream())


def _defer_reduce(job):
    _pending_reduces.append(job)
    # (queued per product, not once per pass: a pass that dies half-way never runs its callbacks, and a flag would then keep the
    # next pass from queueing; the first callback to run does the work, the others find the list empty)
    try:     # runs when the engine has finished this backward pass, with the caller's current stream
        torch.autograd.Variable._execution_engine.queue_callback(flush_deferred_reduces)
    except RuntimeError:     # not inside a backward pass
        flush_deferred_reduces()


def _small(I, J, K, *tensors):
    """Route the product C (I,J) = A (I,K) B (K,J) to fsg_gemm_small_f32?  Yes when both output dimensions are <= 256 --
    the vendor library then runs ONE workgroup and its time grows with I*J*K (tools/probe_vendor_gemm.py) -- and the
    product is big enough for that to cost more than the ~8 us of the small kernel, yet below SMALL_GEMM_FLOPS."""
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
        return False
    vol = float(I) * J * K
    return 0 < I <= 256 and 0 < J <= 256 and (1 << 21) <= vol and 2.0 * vol < SMALL_GEMM_FLOPS


class _LinearPM(torch.autograd.Function):
    """y = x W^T (+ b) over point-major rows.  Large products go to the vendor GEMM (the weight gradient dW = dY^T X, a
    tiny output behind a 16k-long reduction, as a 16-way split-K batched GEMM + a sum: 36-78 us instead of 106-132 us);
    small ones -- everything in the PointTransformer path -- to fsg_gemm_small_f32, because the vendor library runs
    them as a single workgroup."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.pw16 = False
        ctx.fold = _fold_slot(w)
        tw, tb = _grad_targets(w), (_grad_targets(b) if b is not None else ())
        ctx.defer_targets = tw + tb if (tw is not None and tb is not None) else None
        x2 = x.reshape(-1, x.shape[-1])
        N, K = w.shape
        M = x2.shape[0]
        ctx.gs16 = (_bf16_linear and bf16_operands() and M > 0 and
                    all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (x2, w)))
        if ctx.gs16:     # bf16 operand mode: every product of the Linear on fsg_gemm_small_bf16 (same launches as the fp32 route)
            y = gemm_small(x2, K, 1, w, 1, K, b.contiguous() if b is not None else None, M, N, K, bf16=True)
            return y if x.dim() == 2 else y.view(*x.shape[:-1], N)     # (no view of a 2-D result: an in-place ReLU may follow)
        if not (_bf16_linear and bf16_operands()) and _small(M, N, K, x2, w):
            y = gemm_small(x2, K, 1, w, 1, K, b.contiguous() if b is not None else None, M, N, K)
            return y if x.dim() == 2 else y.view(*x.shape[:-1], N)
        ctx.pw16 = _pw_bf16_ok(x2, w)
        if ctx.pw16:     # bf16 operand mode on the hand-written kernel: one bf16 piece per operand, fp32 accumulation
            y = torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=x.device)      # final shape: no view leaves the Function
            pw_linear_bf16(x2, w, b, out=y.view(-1, N))
            return y
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        gx = gw = gb = None
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        if ctx.fold is not None:
            ctx.fold.pending = None
        if ctx.gs16:     # dX = bf16(dY) bf16(W), dW = bf16(dY)^T bf16(X) (+ the bias gradient: row sums of the rounded dY^T)
            N, K = w.shape
            M = g2.shape[0]
            if ctx.needs_input_grad[0]:
                gx = gemm_small(g2, N, 1, w, K, 1, None, M, K, N, bf16=True).view_as(x)
            want_gb = ctx.has_bias and ctx.needs_input_grad[2]
            if ctx.needs_input_grad[1]:
                x2c = x2 if x2.is_contiguous() else x2.contiguous()
                gw = gemm_small(g2, 1, N, x2c, K, 1, None, N, K, M, rowsum=want_gb, defer=_may_defer(ctx.defer_targets), bf16=True)
                if want_gb:
                    gw, gb = gw
            elif want_gb:
                gb = _bias_grad(g2)
            return gx, gw, gb
        if ctx.pw16:     # both gradients on bf16 operands too: dX = bf16(dY) bf16(W), dW = bf16(dY)^T bf16(X)
            if ctx.needs_input_grad[0]:
                gx = (pw_linear_bf16(g2, w.t(), None) if w.shape[0] % 32 == 0 else g2 @ w).view_as(x)
            if ctx.needs_input_grad[1]:
                gw = pw_tn_bf16(g2, x2 if x2.is_contiguous() else x2.contiguous())
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = _bias_grad(g2)
            return gx, gw, gb
        if ctx.needs_input_grad[0]:
            gx = _linear_dx(g2, w).view_as(x)
        want_gb = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] and not want_gb and x2.is_contiguous():
            gw = _dw_unreduced(ctx.fold, w, g2, x2)     # (the first EdgeConv's [P | Q] product: K = 3 input channels)
        if ctx.needs_input_grad[1] and gw is None:
            gw = _linear_dw(g2, x2, with_bias_grad=want_gb, defer=_may_defer(ctx.defer_targets))
            if isinstance(gw, tuple):      # the small-GEMM path hands the bias gradient (row sums of dY^T) over with the product
                gw, gb = gw
        if want_gb and gb is None:
            gb = _bias_grad(g2)
        return gx, gw, gb


def _linear_dx(g2, w, out=None):
    """dX = dY W for dY (M,N), W (N,K); `out`: accumulate into an existing (M,K) gradient instead (one GEMM with beta = 1)"""
    N, K = w.shape
    M = g2.shape[0]
    if out is not None:
        return out.addmm_(g2, w)
    return gemm_small(g2, N, 1, w, K, 1, None, M, K, N) if _small(M, K, N, g2, w) else g2 @ w


def _linear_dw(g2, x2, with_bias_grad=False, defer=False):
    """dW = dY^T X: a tiny output behind a long reduction (see _LinearPM).  with_bias_grad: the small-GEMM path returns
    (dW, db) -- db = column sums of dY as a by-product of the same launch; the other paths return dW alone.
    defer: the caller knows that nothing reads the result inside this backward pass (gemm_small(defer=True))"""
    M, N = g2.shape
    K = x2.shape[1]
    S = 16 if (M % 16 == 0 and M >= 4096) else 1
    if _small(N, K, M, g2, x2):
        return gemm_small(g2, 1, N, x2, K, 1, None, N, K, M, rowsum=with_bias_grad, defer=defer)
    if S > 1 and x2.is_contiguous():
        return torch.bmm(g2.view(S, M // S, -1).transpose(1, 2), x2.view(S, M // S, -1)).sum(0)
    return g2.t() @ x2


_fused_pq_tail = True


def set_fused_pq_tail(flag):
    """Tail of the EdgeConv [P | Q] Linears' backward (default on): their weight gradients dW = dY^T X are left to the backward of
    `edge_weights_many`, which runs all of them in ONE launch (fsg_gemm_small_many_deferred_f32: each product with the tiles and
    splits it has alone) and sums the split partials, in the reduction's own order, inside the launch that transforms them
    (fsg_edge_weights_bwd_folded_f32): the same bits from 2 launches instead of 2 per product + 1.  Off: every product runs and
    reduces at once (the earlier launch sequence; also what every case outside `_dw_unreduced`'s conditions takes).  Returns the
    old value."""
    global _fused_pq_tail
    old, _fused_pq_tail = _fused_pq_tail, bool(flag)
    return old


class _FoldSlot:
    """One weight handed out by `edge_weights_many`, shared between the products that consume it and the Function that made it:
    `uses` counts the products of this forward pass that took the weight; `pending` is (dW tensor, dY, X) of the running backward
    pass while dW is still to be computed.  It holds the TENSORS, so no buffer can be recycled before `_EdgeWeightsMany.backward`
    has consumed them, and it lives and dies with this forward pass's graph: a later pass has slots of its own, and every
    product's backward clears the slot before it decides, so nothing stale is ever picked up."""
    __slots__ = ("uses", "pending")

    def __init__(self):
        self.uses, self.pending = 0, None


def _fold_slot(w):
    """forward of a product with weight `w`: its slot (counted as one more use), or None for any other weight"""
    slot = getattr(w, "_fsg_fold", None)
    if slot is not None:
        slot.uses += 1
    return slot


def _dw_unreduced(slot, w, g2, x2):
    """the tensor that WILL hold dW = dY^T X once `_EdgeWeightsMany.backward` has run, or None when the caller has to compute it at
    once as before: the weight `w` is not one of `edge_weights_many`'s, it feeds a second product (autograd would ADD the two
    gradients -- bytes that are not there yet), it keeps its gradient or carries hooks (they would read it), create_graph
    (gradient mode is on inside such a pass: the gradient may be differentiated, i.e. read), the switch is off, or the product is
    not one fsg_gemm_small_f32 takes.  The tensor returned must reach that backward untouched; it checks."""
    if slot is None:
        return None
    slot.pending = None
    M, N = g2.shape
    K = x2.shape[1]
    if not _fused_pq_tail or slot.uses != 1 or torch.is_grad_enabled() or w.retains_grad or w._backward_hooks or \
            not _small(N, K, M, g2, x2):
        return None
    out = torch.empty(N, K, dtype=torch.float32, device=g2.device)
    slot.pending = (out, g2, x2)
    return out


def _bias_grad(g2):
    """column sums of dY (M,N).  Narrow outputs (the class logits: N = 4) go to fsg_colsum_narrow_f32 -- ATen's dim-0
    reduction of a (16384, 4) tensor takes 17 us; otherwise `sum(0)` (a one-row product with ones is 3-15x slower:
    tools/probe_bias_grad.py)"""
    M, N = g2.shape
    # (one workgroup: worth it up to ~128 K elements -- (16384, 32) takes it 26 us against ATen's 9)
    if g2.is_cuda and g2.dtype == torch.float32 and N <= 32 and (N & (N - 1)) == 0 and 4096 <= M * N <= 131072:
        out = torch.empty(N, dtype=torch.float32, device=g2.device)
        with torch.cuda.device(g2.device):
            _lib.call("fsg_colsum_narrow_f32", _p(g2), M, N, _p(out), _stream())
        return out
    return g2.sum(0)


class _LinearPMGiven(torch.autograd.Function):
    """y = x W^T whose VALUE another kernel has already computed (the previous EdgeConv's apply pass emits the next block's [P | Q]
    rows from the tile it holds in LDS: fsg_edgeconv_apply_pq_f32): the forward hands that tensor through, the backward is the
    ordinary one of the product (dX = dY W, dW = dY^T X)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, w, value):
        ctx.save_for_backward(x, w)
        ctx.fold = _fold_slot(w)
        return value.view_as(value)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        x2 = x.reshape(-1, x.shape[-1])
        gx = _linear_dx(g2, w).view_as(x) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            x2 = x2 if x2.is_contiguous() else x2.contiguous()
            gw = _dw_unreduced(ctx.fold, w, g2, x2)
            if gw is None:
                gw = _linear_dw(g2, x2)
        return gx, gw, None


def linear_pm(x, w, b=None):
    # (routing the EdgeConvs' per-point P/Q products -- M = B N rows, K = 64, N = 128 -- through fsg_pw_linear_f32 /
    # fsg_pw_tn_f32 was measured SLOWER than the vendor GEMM + split-K pair at these sizes: 1.212 vs 1.183 ms per config-2 step,
    # PointTransformer 8.45 vs 8.32 ms -- each product pays its weight-image launch)
    return _LinearPM.apply(x, w, b)


class _LinearPM2(torch.autograd.Function):
    """Two bias-free point-wise layers on the SAME input rows (DGCNNSeg: the global-feature conv 192 -> 1024 and the
    `levels` half of the first head conv 192 -> 256, models/dgcnn.py:134-160): forward as two products, backward with the
    second input gradient accumulated into the first by its GEMM (beta = 1) -- autograd would otherwise add the two
    (M,K) gradients in a kernel of its own."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, w1, w2):
        ctx.save_for_backward(x, w1, w2)
        x2 = x.reshape(-1, x.shape[-1])
        return torch.nn.functional.linear(x2, w1), torch.nn.functional.linear(x2, w2)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g1, g2):
        x, w1, w2 = ctx.saved_tensors
        x2 = x.reshape(-1, x.shape[-1])
        gs = [g.contiguous() if g is not None else None for g in (g1, g2)]
        gx = None
        if ctx.needs_input_grad[0]:
            for g, w in zip(gs, (w1, w2)):
                if g is not None:
                    gx = _linear_dx(g, w) if gx is None else _linear_dx(g, w, out=gx)
            gx = gx.view_as(x) if gx is not None else None
        gw1 = _linear_dw(gs[0], x2) if (gs[0] is not None and ctx.needs_input_grad[1]) else None
        gw2 = _linear_dw(gs[1], x2) if (gs[1] is not None and ctx.needs_input_grad[2]) else None
        return gx, gw1, gw2


def linear_pm2(x, w1, w2):
    """(x W1^T, x W2^T) for x (M,K) contiguous fp32 rows; see _LinearPM2"""
    return _LinearPM2.apply(x, w1, w2)


class _SplitCols(torch.autograd.Function):
    """W (R, C) -> the two column blocks (W[:, :c0], W[:, c0:]) as views (the GEMMs take the row stride); the gradient is
    ONE concatenation.  Slicing a weight twice costs autograd a zero-filled (R, C) tensor + a strided copy per slice and
    an add to merge them."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, w, c0):
        ctx.c0, ctx.c1 = c0, w.shape[1] - c0
        return w[:, :c0], w[:, c0:]

    @staticmethod
    @_amp_bwd
    def backward(ctx, ga, gb):
        if ga is None or gb is None:   # one of the two blocks was not used downstream: its gradient is a zero block
            ref = ga if ga is not None else gb
            ga = ga if ga is not None else torch.zeros(ref.shape[0], ctx.c0, dtype=ref.dtype, device=ref.device)
            gb = gb if gb is not None else torch.zeros(ref.shape[0], ctx.c1, dtype=ref.dtype, device=ref.device)
        return torch.cat([ga, gb], dim=1), None


def split_cols(w, c0):
    return _SplitCols.apply(w, c0)


_ones_memo = {}


def _ones(*shape_and_device):
    """constant ones tensor, memoised (capturable: no fill kernel per call)"""
    *shape, device = shape_and_device
    key = (tuple(shape), str(device))
    t = _ones_memo.get(key)
    if t is None:
        if len(_ones_memo) > 64:
            _ones_memo.clear()
        t = _ones_memo[key] = torch.ones(*shape, dtype=torch.float32, device=device)
    return t


class _AddPerCloud(torch.autograd.Function):
    """y (B,N,C) + c (B,C) broadcast over the points.  The gradient of `c` is the sum over the N points of a cloud; ATen's
    reduction over the middle dimension takes 29 us for (8, 2048, 256), the same sum as a batched one-row product 6 us."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, y, c):
        return y + c.unsqueeze(1)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        B, N, C = g.shape
        gc = g if g.is_contiguous() else g.contiguous()
        return g, torch.bmm(_ones(B, 1, N, g.device), gc).view(B, C)


def add_per_cloud(y, c):
    return _AddPerCloud.apply(y, c)


class _LinearReLU(torch.autograd.Function):
    """relu(x W^T + b) over point-major rows with the bias and the ReLU in the GEMM's epilogue (`torch._addmm_activation`:
    hipBLASLt RELU_BIAS, bit-identical to linear + relu and 16 % faster at 32768 x 512 x 512 -- no separate pass over the
    output); backward masks the gradient once and reuses the routing of `_LinearPM`."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1])
        out = torch._addmm_activation(b, x2, w.t(), use_gelu=False)
        ctx.save_for_backward(x, w, out)
        return out.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        g2 = torch.ops.aten.threshold_backward(g.reshape(-1, g.shape[-1]).contiguous(), out, 0)
        x2 = x.reshape(-1, x.shape[-1])
        gx = _linear_dx(g2, w).view_as(x) if ctx.needs_input_grad[0] else None
        gw = _linear_dw(g2, x2) if ctx.needs_input_grad[1] else None
        gb = _bias_grad(g2) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


def linear_pm_relu(x, w, b):
    """relu(linear(x, w, b)) for fp32 GPU rows, bias required; see _LinearReLU"""
    _need_gpu(x, w, b)
    return _LinearReLU.apply(x, w, b)


class _FoldLayer1(torch.autograd.Function):
    """First layer of a folding MLP (models/folding_net.py:205-221) after the per-cloud part has been split off:
    [relu]( per_cloud[b] + pts[b,i,:] W_p^T ) in ONE pass that writes the (B,m,Cout) activation once
    (fsg_fold_layer1_f32; as thin GEMM + broadcast add + ReLU the tensor is written three times and read twice)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pts, w_p, per_cloud, relu):
        pts, per_cloud = _f32c(pts), _f32c(per_cloud)
        B, m, cp = pts.shape
        Cout = w_p.shape[0]
        if w_p.dtype != torch.float32 or w_p.stride(1) != 1:
            w_p = w_p.float().contiguous()
        out = torch.empty(B, m, Cout, dtype=torch.float32, device=pts.device)
        with torch.cuda.device(pts.device):
            _lib.call("fsg_fold_layer1_f32", _p(pts), cp, _p(w_p), w_p.stride(0), _p(per_cloud), B, m, Cout, int(relu), _p(out),
                      _stream())
        ctx.save_for_backward(pts, w_p, out)
        ctx.relu = bool(relu)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        pts, w_p, out = ctx.saved_tensors
        B, m, cp = pts.shape
        Cout = w_p.shape[0]
        g = g.contiguous()
        if ctx.relu:
            g = torch.ops.aten.threshold_backward(g, out, 0)
        g2 = g.view(B * m, Cout)
        g_pts = (g2 @ w_p).view(B, m, cp) if ctx.needs_input_grad[0] else None
        g_w = _linear_dw(g2, pts.view(B * m, cp)) if ctx.needs_input_grad[1] else None
        g_pc = torch.bmm(_ones(B, 1, m, g.device), g).view(B, Cout) if ctx.needs_input_grad[2] else None
        return g_pts, g_w, g_pc, None


def fold_layer1(pts, w_p, per_cloud, relu=True):
    """pts (B,m,cp<=3), w_p (Cout,cp) (may be a column slice of the conv weight), per_cloud (B,Cout) -> (B,m,Cout)"""
    _need_gpu(pts, w_p, per_cloud)
    return _FoldLayer1.apply(pts, w_p, per_cloud, relu)


class _EdgeWeights(torch.autograd.Function):
    """W = [W_rel | W_ctr] (Co, 2C) -> [W_rel ; W_ctr - W_rel] (2Co, C): the P/Q form of the first EdgeConv layer; one
    launch forward and one backward (fsg_edge_weights_*; ATen's slice / subtract / cat chain is 2 + 4)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, W):
        Co, C2 = W.shape
        Wc = W if (W.dtype == torch.float32 and W.is_contiguous()) else W.float().contiguous()
        out = torch.empty(2 * Co, C2 // 2, dtype=torch.float32, device=W.device)
        with torch.cuda.device(W.device):
            _lib.call("fsg_edge_weights_fwd_f32", _p(Wc), Co, C2 // 2, _p(out), _stream())
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        Co, C = g.shape[0] // 2, g.shape[1]
        gc = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        out = torch.empty(Co, 2 * C, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.call("fsg_edge_weights_bwd_f32", _p(gc), Co, C, _p(out), _stream())
        return out


class _EdgeWeightsMany(torch.autograd.Function):
    """`_EdgeWeights` for all EdgeConv layers of a model in one launch each way: the transforms depend on the weights
    only, so they can run together at the head of the forward -- and, because autograd runs a node once all its output
    gradients are in, together at the tail of the backward."""

    @staticmethod
    def _run(srcs, shapes, backward):
        dev = srcs[0].device
        jobs = _lib.EdgeWeightJobs()
        jobs.n = len(srcs)
        outs = []
        for j, (t, (Co, C)) in enumerate(zip(srcs, shapes)):
            out = torch.empty((Co, 2 * C) if backward else (2 * Co, C), dtype=torch.float32, device=dev)
            jobs.src[j], jobs.dst[j], jobs.Co[j], jobs.C[j] = t.data_ptr(), out.data_ptr(), Co, C
            outs.append(out)
        with torch.cuda.device(dev):
            _lib.call("fsg_edge_weights_many_f32", ctypes.byref(jobs), int(backward), _stream())
        return outs

    @staticmethod
    @_amp_fwd
    def forward(ctx, slots, *Ws):
        Wc = [W if (W.dtype == torch.float32 and W.is_contiguous()) else W.float().contiguous() for W in Ws]
        ctx.shapes = [(W.shape[0], W.shape[1] // 2) for W in Wc]
        ctx.slots = slots
        return tuple(_EdgeWeightsMany._run(Wc, ctx.shapes, False))

    @staticmethod
    @_amp_bwd
    def backward(ctx, *gs):
        dev = next(g for g in gs if g is not None).device
        gc = [torch.zeros(2 * Co, C, dtype=torch.float32, device=dev) if g is None else
              (g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous())
              for g, (Co, C) in zip(gs, ctx.shapes)]
        pending = [None] * len(gc)
        for j, slot in enumerate(ctx.slots or ()):
            pending[j], slot.pending = slot.pending, None
        if not any(pending):
            return (None,) + tuple(_EdgeWeightsMany._run(gc, ctx.shapes, True))
        # weight gradients left to this node (_dw_unreduced): all their products in one launch, then one launch that sums the split
        # partials before it transforms
        prods = _lib.GemmSmallJobs()
        spaces = []
        for j, pend in enumerate(pending):
            if pend is None:
                continue
            dw, g2, x2 = pend
            if gs[j] is None or gs[j].data_ptr() != dw.data_ptr():
                raise RuntimeError("edge_weights_many: the gradient of weight %d is not the product that was registered for it "
                                   "(a weight of edge_weights_many may feed one product only)" % j)
            (M, N), K, i = g2.shape, x2.shape[1], len(spaces)
            ws = _lib.workspace("fsg_gemm_small", N, K, M, device=dev)
            prods.A[i], prods.sa_i[i], prods.sa_k[i], prods.B[i], prods.sb_k[i], prods.sb_j[i] = g2.data_ptr(), 1, N, x2.data_ptr(), K, 1
            prods.C[i], prods.ldc[i], prods.I[i], prods.J[i], prods.K[i] = dw.data_ptr(), K, N, K, M
            prods.workspace[i] = ws.data_ptr() if ws is not None else None
            spaces.append((j, ws))
        prods.n = len(spaces)
        jobs = _lib.EdgeWeightFoldJobs()
        jobs.n = len(gc)
        outs = []
        with torch.cuda.device(dev):
            _lib.call("fsg_gemm_small_many_deferred_f32", ctypes.byref(prods), _stream())
            partials = {j: (ws, prods.splits[i]) for i, (j, ws) in enumerate(spaces)}
            for j, (g, (Co, C)) in enumerate(zip(gc, ctx.shapes)):
                ws, S = partials.get(j, (None, 0))
                out = torch.empty(Co, 2 * C, dtype=torch.float32, device=dev)
                jobs.src[j], jobs.dst[j] = (ws if S > 1 else g).data_ptr(), out.data_ptr()
                jobs.Co[j], jobs.C[j], jobs.S[j] = Co, C, S
                outs.append(out)
            _lib.call("fsg_edge_weights_bwd_folded_f32", ctypes.byref(jobs), _stream())
        return (None,) + tuple(outs)


def edge_weights_many(conv_weights):
    """[(Co,2C,1,1) or (Co,2C) first-layer EdgeConv weights] -> [(2Co,C) P/Q weights], one launch (up to 8 layers)"""
    Ws = [w.reshape(w.shape[0], w.shape[1]) for w in conv_weights]
    if not 1 <= len(Ws) <= 8:
        raise ValueError("edge_weights_many: 1..8 layers")
    slots = [_FoldSlot() for _ in Ws]
    outs = list(_EdgeWeightsMany.apply(slots, *Ws))
    for w, slot in zip(outs, slots):     # marks the weight for the products that take it (_fold_slot)
        w._fsg_fold = slot
    return outs


# ------------------------------------------------------------------ BatchNorm call counters
_deferred_counters = None


def bump_bn_counter(bn):
    """`num_batches_tracked += 1` as torch's BatchNorm does on every training call; returns the momentum of this call.
    Inside `deferred_bn_counters()` the increments of a whole forward are issued as ONE multi-tensor add instead of one
    tiny kernel per BatchNorm (8 per DGCNN-seg step)."""
    if bn.momentum is None:                       # cumulative average: the value is needed now
        bn.num_batches_tracked.add_(1)
        return 1.0 / float(bn.num_batches_tracked)
    if _deferred_counters is not None:
        _deferred_counters.append(bn.num_batches_tracked)
    else:
        bn.num_batches_tracked.add_(1)
    return bn.momentum


@_contextlib.contextmanager
def deferred_bn_counters():
    global _deferred_counters
    if _deferred_counters is not None:            # nested: the outermost context flushes
        yield
        return
    _deferred_counters = []
    try:
        yield
    finally:
        pending, _deferred_counters = _deferred_counters, None
        if pending:
            torch._foreach_add_(pending, 1)


def with_deferred_bn_counters(forward):
    """decorator for a top-level model forward: one multi-tensor add for the BatchNorm call counters, and the whole
    forward outside any ambient autocast region (the plain torch glue between the HIP stages -- concatenations, the small
    per-cloud products -- would otherwise round to fp16 between fp32 kernels); a half-precision input is widened."""
    import functools

    @functools.wraps(forward)
    def wrapped(self, x, *args, **kwargs):
        mode = mfma_operands("bf16") if (x.is_cuda and _ambient_bf16()) else _contextlib.nullcontext()
        with deferred_bn_counters(), mode, no_autocast():
            if torch.is_tensor(x) and x.is_floating_point() and x.dtype != torch.float32:
                x = x.float()
            return forward(self, x, *args, **kwargs)
    return wrapped


def _bn_step(bn):
    """training flag + momentum of one BatchNorm module for this call (bumps num_batches_tracked like torch)."""
    training = bn.training or bn.running_mean is None
    momentum = 0.0
    if training and bn.track_running_stats and bn.num_batches_tracked is not None:
        momentum = bump_bn_counter(bn)
    return training, float(momentum)


def _bn_args(bn):
    """one BatchNorm module -> (weight, bias, running_mean | None, running_var | None, training, momentum, eps) of this call:
    the running statistics are handed on when the call updates them (training, tracked) or reads them (eval)"""
    if bn.weight is None or bn.bias is None:
        raise ValueError("the fused BatchNorm stages need weight and bias: got a BatchNorm with affine=False")
    training, momentum = _bn_step(bn)
    stats = bn.track_running_stats or not training
    return (bn.weight, bn.bias, bn.running_mean if stats else None, bn.running_var if stats else None, training, momentum,
            float(bn.eps))


def _bn_eval_stats(rm, rv, eps):
    """(mean, invstd) of an eval-mode BatchNorm from its running statistics"""
    return rm.detach().float().contiguous(), torch.rsqrt(rv.detach().float() + eps).contiguous()


# ------------------------------------------------------------------ fused EdgeConv (models/dgcnn.py:234-241)
# (the reverse graphs are built on the main stream: building them on a side stream during the forward was MEASURED SLOWER inside
# the replayed hipGraph -- 2.06 vs 1.83 ms/step on MI355X: the fork/join edges cost more than the ~30 us builder hides)
def _build_csr(idx):
    B, N, k = idx.shape
    rowptr = torch.empty(B, N + 1, dtype=torch.int32, device=idx.device)
    col = torch.empty(B, N * k, dtype=torch.int32, device=idx.device)
    ws = _lib.workspace("fsg_graph_reverse_csr", B, N, k, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.call("fsg_graph_reverse_csr", _p(idx), B, N, k, _p(rowptr), _p(col), _p(ws), _stream())
    return rowptr, col


def knn_prep_workspace(B, N, C, device):
    """workspace for a graph build over (B, C, N) points whose PRODUCER prepares it (edgeconv1 / edgeconv2 with knn_ws=, then
    knn_graph(..., prepared=(ws, x_pm))); None when the shape is outside the prepared path (then build the graph as usual)"""
    if C != 64 or N % 64 != 0 or not (1024 <= N <= 8192):
        return None
    return _lib.workspace("fsg_knn_dense", B, N, C, device=device)


def build_reverse_graphs(graphs):
    """Reverse graphs (CSR by destination) of several kNN graphs of the same shape in ONE set of launches instead of one per
    graph: `graphs` are the (B,N,k) slices, in order, of one contiguous (G,B,N,k) buffer (knn_graph(..., out=slice)).  The
    results are cached on the slice tensors exactly as reverse_graph() would (3 x 3 small launches -> 3 per DGCNN-seg step)."""
    g0 = graphs[0]
    G = len(graphs)
    B, N, k = g0.shape
    step = B * N * k * g0.element_size()
    if any(g.shape != g0.shape or g.data_ptr() != g0.data_ptr() + i * step or not g.is_contiguous() for i, g in enumerate(graphs)):
        return          # not one buffer (e.g. graphs substituted by a test): each is built on first use by reverse_graph()
    if all(getattr(g, "_fsg_csr", None) is not None for g in graphs):
        return
    flat = torch.as_strided(g0, (G * B, N, k), (N * k, k, 1))
    rowptr, col = _build_csr(flat)
    for i, g in enumerate(graphs):
        g._fsg_csr = (rowptr[i * B:(i + 1) * B], col[i * B:(i + 1) * B])


def reverse_graph(idx):
    """CSR-by-destination of a kNN graph, cached on the index tensor (a static graph is shared by all layers)."""
    cached = getattr(idx, "_fsg_csr", None)
    if cached is None:
        cached = idx._fsg_csr = _build_csr(idx)
    return cached


def _pm_grad(g, B, N, C):
    """point-major output gradient (B,N,C) -> (tensor, row stride) for the kernels: rows of C contiguous floats with ANY
    row stride pass as they are (e.g. a slice of the gradient of concatenated features), everything else is copied"""
    if g is None:
        return None, 0
    if g.dtype == torch.float32 and g.shape == (B, N, C) and g.stride(2) == 1 and g.stride(1) >= C and \
            (B == 1 or g.stride(0) == N * g.stride(1)):
        return g, g.stride(1)
    return _f32c(g), C


def _apply_pass(ysel, gamma, beta, mean, invstd, B, N, Co, slope, out, out_pm, knn_ws, w_next):
    """the BatchNorm + LeakyReLU pass of a fused EdgeConv when it also prepares the next layer's graph build (knn_ws) and, with
    w_next (128, 64), emits the next fused EdgeConv's [P | Q] rows (returned; else None).  Inside a `with torch.cuda.device`."""
    if knn_ws is None:
        return None
    nb = knn_ws.numel() * knn_ws.element_size()
    if w_next is not None and Co == 64 and tuple(w_next.shape) == (128, 64):
        w_next = _f32c(w_next.detach())
        pq_next = torch.empty(B, N, 128, dtype=torch.float32, device=ysel.device)
        _lib.call("fsg_edgeconv_apply_pq_f32", _p(ysel), _p(gamma), _p(beta), _p(mean), _p(invstd), B, N, Co, slope, _p(out),
                  _p(out_pm), _p(knn_ws), nb, _p(w_next), 128, _p(pq_next), _stream())
        return pq_next
    _lib.call("fsg_edgeconv_apply_f32", _p(ysel), _p(gamma), _p(beta), _p(mean), _p(invstd), B, N, Co, slope, _p(out),
              _p(out_pm), _p(knn_ws), nb, _stream())
    return None


class _EdgeConv1(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, pq, idx, gamma, beta, running_mean, running_var, training, momentum, eps, slope, knn_ws=None, w_next=None):
        pq = _f32c(pq)
        B, N, two_co = pq.shape
        Co, k, dev = two_co // 2, idx.shape[2], pq.device
        gamma, beta = _f32c(gamma), _f32c(beta)
        out = torch.empty(B, Co, N, dtype=torch.float32, device=dev)
        out_pm = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
        ysel = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
        arg = torch.empty(B, N, Co, dtype=torch.uint8, device=dev)
        if training:
            ssum = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
            mean = torch.empty(Co, dtype=torch.float32, device=dev)
            invstd = torch.empty(Co, dtype=torch.float32, device=dev)
            ws = _lib.workspace("fsg_edgeconv1", B, N, Co, device=dev)
        else:
            ssum, ws = None, None
            mean, invstd = _bn_eval_stats(running_mean, running_var, eps)
        with torch.cuda.device(dev):
            _lib.call("fsg_edgeconv1_fwd_f32", _p(pq), _p(idx), _p(gamma), _p(beta),
                      _p(running_mean if training else None), _p(running_var if training else None), B, N, k, Co,
                      int(training), momentum, eps, slope, _p(None if knn_ws is not None else out), _p(out_pm), _p(ysel), _p(arg),
                      _p(ssum), _p(mean), _p(invstd), _p(ws), _stream())
            pq_next = _apply_pass(ysel, gamma, beta, mean, invstd, B, N, Co, slope, out, out_pm, knn_ws, w_next)
        ctx.save_for_backward(pq, idx, gamma, beta, mean, invstd, ysel, arg, ssum)
        ctx.meta = (B, N, k, Co, bool(training), slope)
        ctx.set_materialize_grads(False)   # the layout that only feeds the next graph build gets None, not a zero tensor
        # the point-major output twice (second one an alias): two consumers -- the next layer and the concatenated
        # features -- then deliver their gradients separately and the backward kernel sums them (no ATen add, no copy)
        if pq_next is None:
            return out, out_pm, out_pm.view(B, N, Co)
        ctx.mark_non_differentiable(pq_next)     # (its gradient arrives through _LinearPMGiven on out_pm and the weight)
        return out, out_pm, out_pm.view(B, N, Co), pq_next

    @staticmethod
    @_amp_bwd
    def backward(ctx, g, g_pm, g_pm2, _g_pq_next=None):
        pq, idx, gamma, beta, mean, invstd, ysel, arg, ssum = ctx.saved_tensors
        B, N, k, Co, training, slope = ctx.meta
        dev = pq.device
        g = _f32c(g) if g is not None else None
        g_pm, ld1 = _pm_grad(g_pm, B, N, Co)
        g_pm2, ld2 = _pm_grad(g_pm2, B, N, Co)
        rowptr, col = reverse_graph(idx)
        gpq = torch.empty_like(pq)
        dgamma = torch.empty(Co, dtype=torch.float32, device=dev)
        dbeta = torch.empty(Co, dtype=torch.float32, device=dev)
        h = torch.empty(B, N, Co, dtype=torch.float32, device=dev)
        ws = torch.empty(B * ((N + 63) // 64) * 2 * Co, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_edgeconv1_bwd_f32", _p(g), _p(g_pm), ld1, _p(g_pm2), ld2, _p(pq), _p(rowptr), _p(col), _p(gamma),
                      _p(beta), _p(mean),
                      _p(invstd), _p(ysel), _p(arg), _p(ssum), B, N, k, Co, int(training), slope, _p(gpq), _p(dgamma),
                      _p(dbeta), _p(h), _p(ws), _stream())
        return gpq, None, dgamma, dbeta, None, None, None, None, None, None, None, None


def edgeconv1_supported(out_channels, k):
    return out_channels % 64 == 0 and k <= 64


def edgeconv1(x, idx, conv_weight, bn, slope, x_pm=None, both=False, w_cat=None, knn_ws=None, w_next=None, pq_given=None):
    """Fused single-layer EdgeConv: x (B,C,N), idx (B,N,k) int32, conv_weight (Co,2C,1,1), bn a BatchNorm2d module
    (its running statistics are updated in place like nn.BatchNorm2d does) -> (B,Co,N); with both=True also the
    point-major copy (B,N,Co).  x_pm: optional point-major (B,N,C) copy of x (saves the transpose for the GEMM)."""
    _need_gpu(x, idx, conv_weight)
    Co, C2 = conv_weight.shape[0], conv_weight.shape[1]
    C = C2 // 2
    if w_cat is None:        # (2Co, C): [W_rel ; W_ctr - W_rel]; models hand in the batch of edge_weights_many instead
        w_cat = _EdgeWeights.apply(conv_weight.reshape(Co, C2).to(torch.float32))
    if x_pm is None:
        x_pm = x.transpose(1, 2)
    if pq_given is not None:    # emitted by the previous block's apply pass (w_next): no GEMM launch, ordinary backward
        pq = _LinearPMGiven.apply(x_pm.to(torch.float32), w_cat, pq_given)
    else:
        pq = linear_pm(x_pm.to(torch.float32).contiguous(), w_cat)               # (B,N,2Co): one plain GEMM
    bn_args = _bn_args(bn)
    if idx.dtype != torch.int32:
        idx = idx.to(torch.int32)
    idx = idx.contiguous()
    res = _EdgeConv1.apply(pq, idx, *bn_args, float(slope), knn_ws, w_next if knn_ws is not None else None)
    return _edgeconv_outputs(res, both, w_next is not None)


class _EdgeConv2(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, pq, idx, w2, g1, b1, rm1, rv1, g2, b2, rm2, rv2, training, mom1, mom2, eps1, eps2, slope, knn_ws=None,
                w_next=None):
        pq, w2 = _f32c(pq), _f32c(w2)
        g1, b1, g2, b2 = _f32c(g1), _f32c(b1), _f32c(g2), _f32c(b2)
        B, N, _ = pq.shape
        C2, k, dev = w2.shape[0], idx.shape[2], pq.device

        def new(*shape, dtype=torch.float32):
            return torch.empty(*shape, dtype=dtype, device=dev)
        out, out_pm = new(B, C2, N), new(B, N, C2)
        ysel2, arg2 = new(B, N, C2), new(B, N, C2, dtype=torch.uint8)
        if training:
            ssum1, ssum2 = new(B, N, 64), new(B, N, C2)
            mean1, invstd1, mean2, invstd2 = new(64), new(64), new(C2), new(C2)
        else:
            ssum1 = ssum2 = None
            mean1, invstd1 = _bn_eval_stats(rm1, rv1, eps1)
            mean2, invstd2 = _bn_eval_stats(rm2, rv2, eps2)
        ws = _lib.workspace("fsg_edgeconv2", B, N, k, C2, device=dev)
        t = bool(training)
        ctx.bf16 = bf16_operands()
        with torch.cuda.device(dev):
            _lib.call("fsg_edgeconv2_fwd_bf16" if ctx.bf16 else "fsg_edgeconv2_fwd_f32", _p(pq), _p(idx), _p(w2), _p(g1), _p(b1),
                      _p(rm1 if t else None),
                      _p(rv1 if t else None), _p(g2), _p(b2), _p(rm2 if t else None), _p(rv2 if t else None), B, N, k, C2,
                      int(t), mom1, mom2, eps1, eps2, slope, _p(None if knn_ws is not None else out), _p(out_pm), _p(ssum1), _p(mean1),
                      _p(invstd1), _p(ysel2), _p(arg2), _p(ssum2), _p(mean2), _p(invstd2), _p(ws), _stream())
            pq_next = _apply_pass(ysel2, g2, b2, mean2, invstd2, B, N, C2, slope, out, out_pm, knn_ws, w_next)
        ctx.save_for_backward(pq, idx, w2, g1, b1, mean1, invstd1, ssum1, g2, b2, mean2, invstd2, ysel2, arg2)
        ctx.meta = (B, N, k, C2, t, slope)
        ctx.set_materialize_grads(False)
        if pq_next is None:
            return out, out_pm, out_pm.view(B, N, C2)    # alias for a second consumer, see _EdgeConv1
        ctx.mark_non_differentiable(pq_next)
        return out, out_pm, out_pm.view(B, N, C2), pq_next

    @staticmethod
    @_amp_bwd
    def backward(ctx, g, g_pm, g_pm2, _g_pq_next=None):
        pq, idx, w2, g1, b1, mean1, invstd1, ssum1, g2, b2, mean2, invstd2, ysel2, arg2 = ctx.saved_tensors
        B, N, k, C2, training, slope = ctx.meta
        dev = pq.device
        g = _f32c(g) if g is not None else None
        g_pm, ld1 = _pm_grad(g_pm, B, N, C2)
        g_pm2, ld2 = _pm_grad(g_pm2, B, N, C2)
        rowptr, col = reverse_graph(idx)
        gpq, gw2 = torch.empty_like(pq), torch.empty_like(w2)
        dg1, db1 = torch.empty_like(g1), torch.empty_like(b1)
        dg2, db2 = torch.empty_like(g2), torch.empty_like(b2)
        ws = _lib.workspace("fsg_edgeconv2_bwd", B, N, k, C2, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_edgeconv2_bwd_bf16" if ctx.bf16 else "fsg_edgeconv2_bwd_f32", _p(g), _p(g_pm), ld1, _p(g_pm2), ld2,
                      _p(pq), _p(idx), _p(rowptr), _p(col),
                      _p(w2), _p(g1),
                      _p(b1), _p(mean1), _p(invstd1), _p(ssum1), _p(g2), _p(b2), _p(mean2), _p(invstd2), _p(ysel2),
                      _p(arg2), B, N, k, C2, int(training), slope, _p(gpq), _p(gw2), _p(dg1), _p(db1), _p(dg2), _p(db2),
                      _p(ws), _stream())
        return (gpq, None, gw2, dg1, db1, None, None, dg2, db2) + (None,) * 10


def edgeconv2_supported(c_mid, c_out, k):
    return c_mid == 64 and c_out in (64, 128) and k <= 64


def _edgeconv_outputs(res, both, want_pq_next):
    """(out, out_pm, alias[, pq_next]) of a fused EdgeConv Function -> what the module interface hands out; with w_next given the
    next block's rows come last (None when the pass could not emit them: no knn workspace, other widths)"""
    out, out_pm, out_pm2 = res[:3]
    pq_next = res[3] if len(res) > 3 else None
    if both == "twice":      # (B,Co,N), (B,N,Co) and an alias of the latter for a second consumer (see _EdgeConv1)
        r = (out, out_pm, out_pm2)
    elif both:
        r = (out, out_pm)
    else:
        r = (out,)
    if want_pq_next:
        return r + (pq_next,)
    return r if len(r) > 1 else r[0]


def edgeconv2(x, idx, conv1_weight, bn1, conv2_weight, bn2, slope, x_pm=None, both=False, w_cat=None, knn_ws=None, w_next=None,
              pq_given=None):
    """Fused two-layer EdgeConv (2C -> 64 -> 64|128): see csrc/edgeconv2.hip."""
    _need_gpu(x, idx, conv1_weight, conv2_weight)
    C1, CC = conv1_weight.shape[0], conv1_weight.shape[1]
    C = CC // 2
    if w_cat is None:
        w_cat = _EdgeWeights.apply(conv1_weight.reshape(C1, CC).to(torch.float32))
    if x_pm is None:
        x_pm = x.transpose(1, 2)
    if pq_given is not None:
        pq = _LinearPMGiven.apply(x_pm.to(torch.float32), w_cat, pq_given)
    else:
        pq = linear_pm(x_pm.to(torch.float32).contiguous(), w_cat)               # (B,N,128)
    w2 = conv2_weight.reshape(conv2_weight.shape[0], C1)
    t1, m1 = _bn_step(bn1)
    t2, m2 = _bn_step(bn2)
    if t1 != t2:
        raise RuntimeError("edgeconv2: both BatchNorm layers must be in the same mode")
    if idx.dtype != torch.int32:
        idx = idx.to(torch.int32)
    idx = idx.contiguous()
    res = _EdgeConv2.apply(pq, idx, w2, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var,
                           bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, t1, m1, m2,
                           float(bn1.eps), float(bn2.eps), float(slope), knn_ws, w_next if knn_ws is not None else None)
    return _edgeconv_outputs(res, both, w_next is not None)


# ------------------------------------------------------------------ point-wise layers on the bf16 matrix pipe, fp32-grade
def pw_weight_image(w, scale=1.0, out=None, ks0=0, KS=None):
    """(N, K) fp32 weight (any strides: a view of a wider matrix, or a transposed view) -> the three-piece bf16 operand image of
    csrc/pointwise.hip (include/fsg_hip.h: fsg_pw_weight_image_f32).  `out` / `ks0` / `KS`: fill k-steps [ks0, ks0 + K/16) of
    an existing image that concatenates several matrices along k."""
    _need_gpu(w)
    N, K = w.shape
    ks = (K + 15) // 16
    KS = ks if KS is None else KS
    if out is None:
        out = torch.empty(((N + 31) // 32) * KS * 3 * 1024, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("fsg_pw_weight_image_f32", _p(w), w.stride(0), w.stride(1), N, K, float(scale), ks0, KS, _p(out), _stream())
    return out


def pw_weight_images(specs):
    """several weight images in ONE launch: specs = [(w (N, K) view, scale, out uint8 tensor or None, ks0, KS or None), ...];
    returns the image tensors (include/fsg_hip.h: fsg_pw_weight_images_f32)"""
    jobs = _lib.PWImageJobs()
    outs = []
    assert 1 <= len(specs) <= _lib.PW_MAX_IMAGE_JOBS
    for j, (w, scale, out, ks0, KS) in enumerate(specs):
        N, K = w.shape
        KS = (K + 15) // 16 if KS is None else KS
        if out is None:
            out = torch.empty(((N + 31) // 32) * KS * 3 * 1024, dtype=torch.uint8, device=w.device)
        jobs.W[j], jobs.stride_n[j], jobs.stride_k[j], jobs.N[j], jobs.K[j] = w.data_ptr(), w.stride(0), w.stride(1), N, K
        jobs.ks0[j], jobs.KS[j], jobs.scale[j], jobs.image[j] = ks0, KS, float(scale), out.data_ptr()
        outs.append(out)
    jobs.n = len(specs)
    with torch.cuda.device(specs[0][0].device):
        _lib.call("fsg_pw_weight_images_f32", ctypes.byref(jobs), _stream())
    return outs


# bf16 operands for the nn.Linear products (forward, dX, dW on fsg_pw_linear_bf16 / fsg_pw_tn_bf16) are a SEPARATE opt-in of the
# bf16 mode: measured on the PointTransformer (BASELINE config 3, 2 x 2048 points against the fp32 oracle) they cost accuracy --
# mean |logit error| 0.095, max 0.86, parameter-gradient cosine 0.36 through its 60 BatchNorms and 18 softmax layers -- and time
# (9.0 vs 8.3 ms per step: three more small launches per Linear).  set_bf16_linear(True) / bench.py --workload c3 --dtype bf16
# switch them on.
_bf16_linear = False


def set_bf16_linear(flag):
    """bf16 operands for nn.Linear products while the bf16 operand mode is on (see above); returns the old value"""
    global _bf16_linear
    old, _bf16_linear = _bf16_linear, bool(flag)
    return old


def _pw_bf16_ok(x2, w):
    """bf16 Linear products requested, and the product inside the envelope of fsg_pw_linear_bf16 (fp32 GPU rows, K % 32 == 0)"""
    return (_bf16_linear and bf16_operands() and x2.is_cuda and x2.dtype == torch.float32 and w.dtype == torch.float32 and x2.dim() == 2 and
            x2.stride(1) == 1 and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0 and x2.shape[1] % 32 == 0 and x2.shape[0] > 0)


def pw_linear_bf16(x, w, bias=None, tile=0, out=None):
    """y (M, N) = bf16(x) bf16(w)^T (+ bias), fp32 accumulation: one-piece mode of csrc/pointwise.hip (include/fsg_hip.h:
    fsg_pw_weight_image_bf16 + fsg_pw_linear_bf16).  w (N, K): any strides (a transposed view gives dX = dY W)."""
    M, K = x.shape
    N = w.shape[0]
    dev = x.device
    img = torch.empty(((N + 31) // 32) * ((K + 15) // 16) * 1024, dtype=torch.uint8, device=dev)
    y = torch.empty(M, N, dtype=torch.float32, device=dev) if out is None else out
    with torch.cuda.device(dev):
        _lib.call("fsg_pw_weight_image_bf16", _p(w), w.stride(0), w.stride(1), N, K, _p(img), _stream())
        _lib.call("fsg_pw_linear_bf16", _p(x), x.stride(0), _p(img), _p(bias.contiguous() if bias is not None else None), _p(y), N,
                  M, N, K, tile, _stream())
    return y


def pw_tn_bf16(g, x, rows_per_slice=None):
    """dW (N, K) = bf16(g)^T bf16(x) for g (M, N), x (M, K) contiguous rows, fp32 accumulation over the M rows in fixed slice
    order (include/fsg_hip.h: fsg_pw_tn_bf16)"""
    M, N = g.shape
    K = x.shape[1]
    dev = g.device
    if rows_per_slice is None:      # enough slices to fill the chip, never below 64 rows
        tiles = ((N + 63) // 64) * ((K + 63) // 64)
        rows_per_slice = max(64, min(1024, ((M * tiles // 512) // 32) * 32)) if M * tiles >= 512 * 64 else 64
    a = _lib.PWTnArgs()
    a.L1, a.ldl1, a.N1a, a.N1b, a.lpro = g.data_ptr(), g.stride(0), N, 0, 0
    a.R, a.ldr, a.N2, a.rpro = x.data_ptr(), x.stride(0), K, 0
    a.M, a.rows_per_cloud, a.rows_per_slice = M, 0, rows_per_slice
    ws = _lib.workspace("fsg_pw_tn", N, K, M, rows_per_slice, device=dev)
    out = torch.empty(N, K, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fsg_pw_tn_bf16", ctypes.byref(a), 3, _p(ws), ws.numel(), _p(out), K, _stream())
    return out


def pw_linear(x, image, N, bias=None, tile=0):
    """y (M, N) = x (M, K) W^T (+ bias) with W given as pw_weight_image(W): six bf16 MFMA products per fp32 product, fp32
    accumulation (include/fsg_hip.h: fsg_pw_linear_f32)"""
    _need_gpu(x)
    M, K = x.shape
    assert x.stride(1) == 1 and x.dtype == torch.float32
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("fsg_pw_linear_f32", _p(x), x.stride(0), _p(image), _p(bias), _p(y), N, M, N, K, tile, _stream())
    return y

PW_STORE, PW_STATS, PW_SEL, PW_BWDSTATS, PW_BIAS = _lib.PW_STORE, _lib.PW_STATS, _lib.PW_SEL, _lib.PW_BWDSTATS, _lib.PW_BIAS
PRO_NONE, PRO_BNACT, PRO_BNBWD = _lib.PW_PRO_NONE, _lib.PW_PRO_BNACT, _lib.PW_PRO_BNBWD


def _ptr(t):
    return t.data_ptr() if t is not None else None


def pw_rowgemm(pro, epi, tile, **kw):
    """include/fsg_hip.h: fsg_pw_rowgemm_f32 -- keyword arguments are the fields of fsg_pw_rowgemm_args (tensors or numbers)"""
    a = _lib.PWRowGemmArgs()
    keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(a, k, v)
    dev = keep[0].device
    with torch.cuda.device(dev):
        _lib.call("fsg_pw_rowgemm_f32", ctypes.byref(a), pro, epi, tile, _stream())


def pw_rowgemm_scatter(sorted_keys, first, coef, W, **kw):
    """include/fsg_hip.h: fsg_pw_rowgemm_scatter_f32 -- the (PRO_BNBWD, PW_STORE | PW_BIAS, tile 5) product with
    fsg_pw_scatter_rows_f32 in its epilogue; sorted_keys / first: from fsg_pw_gf_prep_sort_f32; keyword arguments as pw_rowgemm"""
    a = _lib.PWRowGemmArgs()
    keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(a, k, v)
    with torch.cuda.device(coef.device):
        _lib.call("fsg_pw_rowgemm_scatter_f32", ctypes.byref(a), _p(sorted_keys), _p(first), _p(coef), _p(W), W.stride(0),
                  coef.shape[1], _stream())


def pw_tn(tile, C1, ldc1, C2=None, ldc2=0, defer=None, **kw):
    """include/fsg_hip.h: fsg_pw_tn_f32.  `defer`: a list -- the slices stay in their workspace and the job is appended to the
    list, to be folded by `pw_tn_reduce(list)` together with the other products' (one launch instead of one per product)"""
    a = _lib.PWTnArgs()
    keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(a, k, v)
    dev = C1.device
    N1 = a.N1a + a.N1b + (1 if a.ones else 0)
    ws = _lib.workspace("fsg_pw_tn", N1, a.N2, a.M, a.rows_per_slice, device=dev)
    with torch.cuda.device(dev):
        if defer is None:
            _lib.call("fsg_pw_tn_f32", ctypes.byref(a), tile, _p(ws), ws.numel(), _p(C1), ldc1, _p(C2), ldc2, _stream())
        else:
            _lib.call("fsg_pw_tn_f32", ctypes.byref(a), tile, _p(ws), ws.numel(), None, 0, None, 0, _stream())
            defer.append((ws, C1, ldc1, C2, ldc2, (a.M + a.rows_per_slice - 1) // a.rows_per_slice, N1, a.N2, a.N1a))


def pw_tn_reduce(jobs):
    """include/fsg_hip.h: fsg_pw_tn_reduce_f32 -- fold the slices of the deferred products of pw_tn, one launch"""
    j = _lib.PWTnReduceJobs()
    assert 1 <= len(jobs) <= _lib.PW_MAX_REDUCE_JOBS
    for i, (ws, C1, ldc1, C2, ldc2, S, N1, N2, N1a) in enumerate(jobs):
        j.workspace[i], j.C1[i], j.ldc1[i], j.C2[i], j.ldc2[i] = ws.data_ptr(), C1.data_ptr(), ldc1, _ptr(C2), ldc2
        j.S[i], j.N1[i], j.N2[i], j.N1a[i] = S, N1, N2, N1a
    j.n = len(jobs)
    with torch.cuda.device(jobs[0][0].device):
        _lib.call("fsg_pw_tn_reduce_f32", ctypes.byref(j), _stream())


def _pw_bn_finalize(rec, R, ldn, c0, C, shift, B, bn, training, momentum, with_emu=False, with_cloud_mean=False, gfeat=None,
                    wglob=None):
    """statistics + consumer tables of one BatchNorm of the fused head; returns (mean, invstd, alpha, delta, emu, cloud_mean).
    `gfeat` (B, CG) + `wglob` (C, CG) view: the per-cloud shift gfeat wglob^T is formed inside the kernel (written to `shift`)"""
    dev = bn.weight.device
    nb = B if shift is not None else 1
    alpha = torch.empty(C, dtype=torch.float32, device=dev)
    delta = torch.empty(nb, C, dtype=torch.float32, device=dev)
    emu = torch.empty(nb, C, dtype=torch.float32, device=dev) if with_emu else None
    cm = torch.empty(B, C, dtype=torch.float32, device=dev) if (with_cloud_mean and training) else None
    if training:
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        track = bn.track_running_stats and bn.running_mean is not None
        rm, rv = (bn.running_mean, bn.running_var) if track else (None, None)
    else:
        mean, invstd = _bn_eval_stats(bn.running_mean, bn.running_var, bn.eps)
        rm = rv = None
    with torch.cuda.device(dev):
        _lib.call("fsg_pw_bn_finalize_f32", _p(rec), R, ldn, c0, C, _p(shift), B, int(training), _p(bn.weight), _p(bn.bias),
                  float(bn.eps), float(momentum), _p(rm), _p(rv), _p(mean), _p(invstd), _p(alpha), _p(delta), _p(emu), _p(cm),
                  _p(gfeat), _p(wglob), wglob.stride(0) if wglob is not None else 0, gfeat.shape[1] if gfeat is not None else 0,
                  _p(shift) if gfeat is not None else None, _stream())
    return mean, invstd, alpha, delta, emu, cm


class _SegHead(torch.autograd.Function):
    """The whole point-wise head of DGCNNSeg behind the three EdgeConvs (models/dgcnn.py:123-162 of the reference) as ONE
    autograd node on the fused kernels of csrc/pointwise.hip:
      levels (M, 192) -> [Wg ; W0_levels] product: BatchNorm statistics + per-cloud max of the 1024 global-feature channels in
      the epilogue (the (M, 1024) activation never exists), y0 stored -> g (B, 1024) -> c = g W0_global^T per cloud ->
      BN0 (statistics of y0 + c[cloud] from the per-cloud records) -> layer 1, layer 2 with BatchNorm + LeakyReLU of the
      producer applied in the prologue and statistics in the epilogue -> class logits.
    Backward: BatchNorm backward formed in the prologues (dy never stored), its sums in the epilogue of the product that makes
    the activation gradient, weight gradients by the row-contraction kernel, the global-feature layer in its Gram form."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, levels, B, Npts, slope, bns, steps, Wg, gg, bg, W0, g0, b0, W1, g1, b1, W2, g2, b2, W3, b3):
        M, KL = levels.shape
        dev = levels.device
        CG, C0, C1, C2, CLS = Wg.shape[0], W0.shape[0], W1.shape[0], W2.shape[0], W3.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        (tr_g, mom_g), (tr_0, mom_0), (tr_1, mom_1), (tr_2, mom_2) = steps
        bn_g, bn_0, bn_1, bn_2 = bns
        # weight images (three bf16 pieces in MFMA operand layout)
        ksl = KL // 16
        img0 = torch.empty(((CG + C0) // 32) * ksl * 3 * 1024, dtype=torch.uint8, device=dev)
        ks_a, ks_b = C0 // 16, KL // 16
        img_lv = torch.empty((KL // 32) * (ks_a + ks_b) * 3 * 1024, dtype=torch.uint8, device=dev)   # [W0_levels^T ; -M1]: backward
        specs = [(Wg, 1.0, img0, 0, None), (W0[:, :KL], 1.0, img0[(CG // 32) * ksl * 3 * 1024:], 0, None), (W1, 1.0, None, 0, None),
                 (W2, 1.0, None, 0, None), (W3, 1.0, None, 0, None)]
        # (forward runs with grad mode off: whether a backward can follow is what the tensors require)
        need_bwd = any(t.requires_grad for t in (levels, Wg, gg, bg, W0, g0, b0, W1, g1, b1, W2, g2, b2, W3) if t is not None) or \
            (b3 is not None and b3.requires_grad)
        if need_bwd:    # transposed images for the backward products ride in the same launch
            specs += [(W2.t(), 1.0, None, 0, None), (W1.t(), 1.0, None, 0, None), (W0[:, :KL].t(), 1.0, img_lv, 0, ks_a + ks_b)]
        imgs = pw_weight_images(specs)
        img1, img2, img3 = imgs[2], imgs[3], imgs[4]
        img2t, img1t = (imgs[5], imgs[6]) if need_bwd else (None, None)
        # levels -> global-feature statistics / selection + y0
        R0 = M // 128
        rec0 = torch.empty(R0, 3, CG + C0, **f32)
        sel_val = torch.empty(R0, CG, **f32)
        sel_arg = torch.empty(R0, CG, dtype=torch.int32, device=dev)
        y0 = torch.empty(M, C0, **f32)
        sgn = gg                     # only the sign of the BatchNorm weight is used (max of sgn * y through the monotone BN + LeakyReLU)
        pw_rowgemm(PRO_NONE, PW_STORE | PW_STATS | PW_SEL, 1, A1=levels, lda1=levels.stride(0), K1=KL, K2=0, Bimg=img0, M=M,
                   N=CG + C0, rows_per_cloud=Npts, C=y0, ldc=C0, store_n0=CG, rec=rec0, sgn=sgn, sel_val=sel_val,
                   sel_arg=sel_arg, sel_n=CG)
        # BatchNorm statistics of the global-feature layer AND the finish of its max-pool (one launch: fsg_pw_bn_finalize_max_f32)
        g = torch.empty(B, CG, **f32)
        ysel = torch.empty(B, CG, **f32)
        arg = torch.empty(B, CG, dtype=torch.int32, device=dev)
        al_g, de_g = torch.empty(CG, **f32), torch.empty(1, CG, **f32)
        if tr_g:
            mean_g, inv_g = torch.empty(CG, **f32), torch.empty(CG, **f32)
            track = bn_g.track_running_stats and bn_g.running_mean is not None
            rm_g, rv_g = (bn_g.running_mean, bn_g.running_var) if track else (None, None)
        else:
            mean_g, inv_g = _bn_eval_stats(bn_g.running_mean, bn_g.running_var, bn_g.eps)
            rm_g = rv_g = None
        with torch.cuda.device(dev):
            _lib.call("fsg_pw_bn_finalize_max_f32", _p(rec0), R0, CG + C0, 0, CG, B, int(tr_g), _p(bn_g.weight), _p(bn_g.bias),
                      float(bn_g.eps), float(mom_g), _p(rm_g), _p(rv_g), _p(mean_g), _p(inv_g), _p(al_g), _p(de_g), _p(sel_val),
                      _p(sel_arg), _p(sgn), Npts // 128, slope, _p(g), _p(ysel), _p(arg), _stream())
        c = torch.empty(B, C0, **f32)     # g W0_global^T: the global part of the first head layer, one wave per output
        with torch.cuda.device(dev):
            _lib.call("fsg_pw_cloud_linear_f32", _p(g), _p(W0[:, KL:]), W0.stride(0), B, C0, CG, _p(c), _stream())
        mean_0, inv_0, al_0, de_0, emu_0, cm_0 = _pw_bn_finalize(rec0, R0, CG + C0, CG, C0, c, B, bn_0, tr_0, mom_0,
                                                                 with_emu=True, with_cloud_mean=True)
        # layer 1, layer 2, logits
        R1 = M // 64
        y1 = torch.empty(M, C1, **f32)
        rec1 = torch.empty(R1, 3, C1, **f32)
        pw_rowgemm(PRO_BNACT, PW_STORE | PW_STATS, 2, A1=y0, lda1=C0, K1=C0, K2=0, Bimg=img1, M=M, N=C1, rows_per_cloud=Npts,
                   alpha=al_0, delta=de_0, tstride=C0, slope=slope, C=y1, ldc=C1, store_n0=0, rec=rec1)
        mean_1, inv_1, al_1, de_1, _, _ = _pw_bn_finalize(rec1, R1, C1, 0, C1, None, B, bn_1, tr_1, mom_1)
        y2 = torch.empty(M, C2, **f32)
        rec2 = torch.empty(R1, 3, C2, **f32)
        pw_rowgemm(PRO_BNACT, PW_STORE | PW_STATS, 3, A1=y1, lda1=C1, K1=C1, K2=0, Bimg=img2, M=M, N=C2, rows_per_cloud=Npts,
                   alpha=al_1, delta=de_1, tstride=0, slope=slope, C=y2, ldc=C2, store_n0=0, rec=rec2)
        mean_2, inv_2, al_2, de_2, _, _ = _pw_bn_finalize(rec2, R1, C2, 0, C2, None, B, bn_2, tr_2, mom_2)
        out = torch.empty(M, CLS, **f32)
        pw_rowgemm(PRO_BNACT, PW_STORE | PW_BIAS, 3, A1=y2, lda1=C2, K1=C2, K2=0, Bimg=img3, M=M, N=CLS, rows_per_cloud=Npts,
                   alpha=al_2, delta=de_2, tstride=0, slope=slope, C=out, ldc=CLS, store_n0=0, bias=b3)
        if not need_bwd:       # inference: nothing kept
            return out
        ctx.images = (img2t, img1t, img_lv)
        ctx.save_for_backward(levels, y0, y1, y2, Wg, W0, W1, W2, W3, g, ysel, arg, c,
                              mean_g, inv_g, al_g, de_g, mean_0, inv_0, al_0, de_0, emu_0,
                              cm_0 if cm_0 is not None else torch.zeros(B, C0, **f32), mean_1, inv_1, al_1, de_1, mean_2, inv_2, al_2, de_2)
        ctx.meta = (B, Npts, slope, (tr_g, tr_0, tr_1, tr_2))
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, gout):
        (levels, y0, y1, y2, Wg, W0, W1, W2, W3, g, ysel, arg, c, mean_g, inv_g, al_g, de_g, mean_0, inv_0, al_0, de_0, emu_0,
         cm_0, mean_1, inv_1, al_1, de_1, mean_2, inv_2, al_2, de_2) = ctx.saved_tensors
        B, Npts, slope, (tr_g, tr_0, tr_1, tr_2) = ctx.meta
        img2t, img1t, img_lv = ctx.images
        M, KL = levels.shape
        dev = levels.device
        CG, C0, C1, C2, CLS = Wg.shape[0], W0.shape[0], W1.shape[0], W2.shape[0], W3.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        gout = gout if gout.is_contiguous() else gout.contiguous()

        def call(name, *a):
            with torch.cuda.device(dev):
                _lib.call(name, *a, _stream())
        # ---- logits layer
        # folded tail (set_fused_head_tail): db3 by one more workgroup of the logits launch, where _bias_grad would take
        # fsg_colsum_narrow_f32 (the same sums in the same order); the key sort + tile table in the launch behind gf_prep and the
        # scatter in the epilogue of the dlv product, where the head takes the 64 x 192 tile and the 1024-key sort
        tail_bias = _fused_head_tail and (CLS & (CLS - 1)) == 0 and 4096 <= M * CLS <= 131072
        tail_scatter = _fused_head_tail and KL == 192 and 512 < CG <= 1024
        db3 = torch.empty(CLS, **f32) if tail_bias else _bias_grad(gout)
        dW3 = torch.empty(CLS, C2, **f32)
        folds = []                      # the four weight-gradient products leave their row slices; one launch folds them at the end
        pw_tn(3, dW3, C2, defer=folds, L1=gout, ldl1=CLS, N1a=CLS, N1b=0, lpro=PRO_NONE, R=y2, ldr=C2, N2=C2, rpro=PRO_BNACT, ralpha=al_2,
              rdelta=de_2, rts=0, slope=slope, M=M, rows_per_cloud=Npts, rows_per_slice=128)
        da2 = torch.empty(M, C2, **f32)
        Rb = (M + 31) // 32
        r2b = torch.empty(Rb, 2, C2, **f32)
        if tail_bias:
            call("fsg_pw_logits_bwd_bias_f32", _p(gout), CLS, _p(W3), _p(y2), _p(al_2), _p(de_2), _p(mean_2), _p(inv_2), M, C2, slope,
                 _p(da2), _p(r2b), _p(db3))
        else:
            call("fsg_pw_logits_bwd_f32", _p(gout), CLS, _p(W3), _p(y2), _p(al_2), _p(de_2), _p(mean_2), _p(inv_2), M, C2, slope,
                 _p(da2), _p(r2b))

        def bwd_fin(rec, R, C, training, alpha, inv, emu, per_cloud, cm=None, want_dc=False):
            nb = B if per_cloud else 1
            dbeta, dgamma = torch.empty(C, **f32), torch.empty(C, **f32)
            P, Q = torch.empty(nb, C, **f32), torch.empty(C, **f32)
            dc = torch.empty(B, C, **f32) if want_dc else None
            call("fsg_pw_bnbwd_finalize_f32", _p(rec), R, C, B, M, int(training), _p(alpha), _p(inv), _p(emu), int(per_cloud),
                 _p(cm), _p(dbeta), _p(dgamma), _p(P), _p(Q), _p(dc))
            return dbeta, dgamma, P, Q, dc
        db2, dg2, P2, Q2, _ = bwd_fin(r2b, Rb, C2, tr_2, al_2, inv_2, mean_2, False)
        # ---- layer 2
        dW2 = torch.empty(C2, C1, **f32)
        pw_tn(2, dW2, C1, defer=folds, L1=da2, LY1=y2, ldl1=C2, N1a=C2, N1b=0, lpro=PRO_BNBWD, lalpha=al_2, ldelta=de_2, lP=P2, lQ=Q2, lts=0,
              R=y1, ldr=C1, N2=C1, rpro=PRO_BNACT, ralpha=al_1, rdelta=de_1, rts=0, slope=slope, M=M, rows_per_cloud=Npts,
              rows_per_slice=_tn_rps(M))
        R1 = M // 64
        da1 = torch.empty(M, C1, **f32)
        r1b = torch.empty(R1, 2, C1, **f32)
        pw_rowgemm(PRO_BNBWD, PW_STORE | PW_BWDSTATS, 2, A1=da2, Y1=y2, lda1=C2, K1=C2, K2=0, Bimg=img2t, M=M,
                   N=C1, rows_per_cloud=Npts, alpha=al_2, delta=de_2, P=P2, Q=Q2, tstride=0, slope=slope, C=da1, ldc=C1,
                   store_n0=0, Yp=y1, ldyp=C1, ealpha=al_1, edelta=de_1, emu=mean_1, er=inv_1, etstride=0, rec2=r1b)
        db1, dg1, P1, Q1, _ = bwd_fin(r1b, R1, C1, tr_1, al_1, inv_1, mean_1, False)
        # ---- layer 1
        dW1 = torch.empty(C1, C0, **f32)
        pw_tn(1, dW1, C0, defer=folds, L1=da1, LY1=y1, ldl1=C1, N1a=C1, N1b=0, lpro=PRO_BNBWD, lalpha=al_1, ldelta=de_1, lP=P1, lQ=Q1, lts=0,
              R=y0, ldr=C0, N2=C0, rpro=PRO_BNACT, ralpha=al_0, rdelta=de_0, rts=C0, slope=slope, M=M, rows_per_cloud=Npts,
              rows_per_slice=_tn_rps(M))
        da0 = torch.empty(M, C0, **f32)
        r0b = torch.empty(R1, 2, C0, **f32)
        pw_rowgemm(PRO_BNBWD, PW_STORE | PW_BWDSTATS, 2, A1=da1, Y1=y1, lda1=C1, K1=C1, K2=0, Bimg=img1t, M=M,
                   N=C0, rows_per_cloud=Npts, alpha=al_1, delta=de_1, P=P1, Q=Q1, tstride=0, slope=slope, C=da0, ldc=C0,
                   store_n0=0, Yp=y0, ldyp=C0, ealpha=al_0, edelta=de_0, emu=emu_0, er=inv_0, etstride=C0, rec2=r0b)
        db0, dg0, P0, Q0, dc = bwd_fin(r0b, R1, C0, tr_0, al_0, inv_0, emu_0, True, cm=cm_0, want_dc=True)
        # ---- first head layer (levels part + per-cloud global part) and the global-feature layer in its Gram form
        dW0 = torch.empty(C0, KL + CG, **f32)
        dbg, dgg = torch.empty(CG, **f32), torch.empty(CG, **f32)
        Pg, Qg, coef = torch.empty(CG, **f32), torch.empty(CG, **f32), torch.empty(B, CG, **f32)
        W0G, dW0G = W0[:, KL:], dW0[:, KL:]
        ldq = (KL + 4) & ~3
        Wq = torch.empty(CG, ldq, **f32)                                   # rows [Q o Wg | -P]
        if tail_scatter:
            skeys = torch.empty(B, 1024, dtype=torch.int32, device=dev)         # sorted (arg << 12 | channel) per cloud
            sfirst = torch.empty(B, Npts // 64 + 1, dtype=torch.int32, device=dev)
            call("fsg_pw_gf_prep_sort_f32", _p(dc), _p(W0G), W0.stride(0), C0, _p(g), _p(dW0G), dW0.stride(0), _p(ysel), _p(al_g),
                 _p(de_g), _p(mean_g), _p(inv_g), B, CG, M, int(tr_g), slope, _p(dbg), _p(dgg), _p(Pg), _p(Qg), _p(coef), _p(Wg),
                 Wg.stride(0), KL, _p(Wq), ldq, _p(arg), Npts, _p(skeys), _p(sfirst))
        else:
            call("fsg_pw_gf_prep_f32", _p(dc), _p(W0G), W0.stride(0), C0, _p(g), _p(dW0G), dW0.stride(0), None, _p(ysel), _p(al_g),
                 _p(de_g), _p(mean_g), _p(inv_g), B, CG, M, int(tr_g), slope, _p(dbg), _p(dgg), _p(Pg), _p(Qg), _p(coef), _p(Wg),
                 Wg.stride(0), KL, _p(Wq), ldq)
        # [M1 ; npvec] = [Q o Wg | -P]^T Wg with M1 = Wg^T diag(Q) Wg: one row contraction over the CG channel rows
        ks_a, ks_b = C0 // 16, KL // 16
        tn_m1 = dict(L1=Wq, ldl1=ldq, N1a=KL + 1, N1b=0, lpro=PRO_NONE, R=Wg, ldr=Wg.stride(0), N2=KL, rpro=PRO_NONE, slope=slope,
                     M=CG, rows_per_cloud=0, rows_per_slice=64)
        if _fused_head_tail:       # the fold writes -M1 straight into the B image; M1 itself is not stored
            npvec = torch.empty(KL, **f32)
            part = []
            pw_tn(3, npvec, KL, defer=part, **tn_m1)
            call("fsg_pw_tn_reduce_image_f32", _p(part[0][0]), part[0][5], KL + 1, KL, KL, -1.0, ks_a, ks_a + ks_b, _p(img_lv),
                 _p(npvec), KL)
        else:
            m1n = torch.empty(KL + 1, KL, **f32)
            pw_tn(3, m1n, KL, **tn_m1)
            M1, npvec = m1n[:KL], m1n[KL]
            pw_weight_image(M1, scale=-1.0, out=img_lv, ks0=ks_a, KS=ks_a + ks_b)
        Gs = torch.empty(KL + 1, KL, **f32)          # [X^T X ; column sums of X] (the all-ones column behind the left operand)
        G, s = Gs[:KL], Gs[KL]
        pw_tn(5, dW0, KL + CG, Gs, KL, defer=folds, ones=1, L1=da0, LY1=y0, L2=levels, ldl1=C0, ldl2=levels.stride(0), N1a=C0, N1b=KL, lpro=PRO_BNBWD,
              lalpha=al_0, ldelta=de_0, lP=P0, lQ=Q0, lts=C0, R=levels, ldr=levels.stride(0), N2=KL, rpro=PRO_NONE, slope=slope,
              M=M, rows_per_cloud=Npts, rows_per_slice=_tn_rps(M))
        pw_tn_reduce(folds)             # dW3, dW2, dW1, [dW0_levels ; G]
        dlv = torch.empty(M, KL, **f32)
        # the 64 x 192 tile (5) for the (B N, 448) x (448, 192) input-gradient product of the first head layer: its BatchNorm-backward
        # prologue + split is then done once per row instead of once per column tile (38.8 -> 33.1 us).  The 64 x 256 tile for the
        # 256-wide products was measured SLOWER (24.9 vs 20.7 us, 25.5 vs 21.3 us: 120 KB of LDS = one workgroup per CU)
        gemm_lv = dict(A1=da0, Y1=y0, A2=levels, lda1=C0, lda2=levels.stride(0), K1=C0, K2=KL, Bimg=img_lv, M=M, N=KL,
                       rows_per_cloud=Npts, alpha=al_0, delta=de_0, P=P0, Q=Q0, tstride=C0, slope=slope, C=dlv, ldc=KL, store_n0=0,
                       bias=npvec)
        if tail_scatter:           # the scatter of the selected rows rides in the product's epilogue
            pw_rowgemm_scatter(skeys, sfirst, coef, Wg, **gemm_lv)
        else:
            pw_rowgemm(PRO_BNBWD, PW_STORE | PW_BIAS, 5 if KL == 192 else 4, **gemm_lv)
            sws = _lib.workspace("fsg_pw_scatter_rows", B, CG, device=dev)
            call("fsg_pw_scatter_rows_f32", _p(coef), _p(arg), _p(Wg), Wg.stride(0), B, CG, KL, Npts, _p(dlv), KL, _p(sws))
        dWg = torch.empty(CG, KL, **f32)
        call("fsg_pw_gf_dw_f32", _p(coef), _p(arg), _p(levels), levels.stride(0), _p(s), _p(Wg), Wg.stride(0), _p(G), _p(Pg), _p(Qg),
             B, CG, KL, Npts, _p(dWg), KL)
        return (dlv, None, None, None, None, None, dWg, dgg, dbg, dW0, dg0, db0, dW1, dg1, db1, dW2, dg2, db2, dW3, db3)


_fused_head = True


def _tn_rps(M):
    """rows per slice of the head's weight-gradient contractions: 128 up to 16384 rows (512 workgroups per product, two resident per
    CU: config 2 0.956 vs 0.960 ms per step at 256, 1.005 at 64), 256 above (config 4: 2.07 vs 2.10 ms at 128; 32 x 2048 static:
    3.19 vs 3.24 -- twice the partial products to write and fold)"""
    return 128 if M <= 16384 else 256


def set_fused_head(flag):
    """switch the fused point-wise head of DGCNNSeg (csrc/pointwise.hip) on / off; off = vendor GEMMs + fsg_bn_act_* stages
    (the round-2 path, kept for shapes outside the fused kernels' envelope and as their cross-check); returns the old value"""
    global _fused_head
    old, _fused_head = _fused_head, bool(flag)
    return old


_fused_head_tail = True


def set_fused_head_tail(flag):
    """the folded tail of the fused head's backward (bias gradient in the logits launch, key sort behind gf_prep, -M1 image
    from the fold, scatter in the dlv product's epilogue: include/fsg_hip.h) on / off; off = the separate launches, which
    also serve the widths outside the folded kernels' envelope.  Both give the same bits.  Returns the old value"""
    global _fused_head_tail
    old, _fused_head_tail = _fused_head_tail, bool(flag)
    return old


def seg_head_supported(levels, B, Npts, Wg, W0, W1, W2, W3, blocks=None):
    """the fused head needs: fp32 GPU rows, clouds of a multiple of 256 points, channel counts on the 32 / 64 grid, at most 32
    clouds per rank (the reference's experiment scripts train with 32); `blocks` = (global block, *segmentation blocks): the
    four BatchNorm-backed blocks must be what models/dgcnn.py:282-323 builds -- conv without bias, AFFINE BatchNorm1d, LeakyReLU
    (the fused node has no place for a conv bias in front of a BatchNorm and reads gamma / beta unconditionally)"""
    if not _fused_head:     # (bf16 operand mode keeps the fused head: its products are fp32-grade, above what the mode asks for)
        return False
    if blocks is not None:
        for blk in blocks[:4]:
            conv, bn, act = blk.layers[0], blk.layers[1], blk.layers[2]
            if (conv.bias is not None or not isinstance(bn, torch.nn.BatchNorm1d) or not bn.affine or
                    not isinstance(act, torch.nn.LeakyReLU)):
                return False
    KL = levels.shape[1]
    return (levels.is_cuda and levels.dtype == torch.float32 and levels.stride(1) == 1 and levels.stride(0) % 4 == 0 and
            Npts % 256 == 0 and levels.shape[0] == B * Npts and KL % 64 == 0 and Wg.shape[0] % 128 == 0 and
            W0.shape[0] % 64 == 0 and W0.shape[1] == KL + Wg.shape[0] and W1.shape[0] % 64 == 0 and W1.shape[1] == W0.shape[0] and
            W2.shape[0] % 64 == 0 and W2.shape[1] == W1.shape[0] and W3.shape[1] == W2.shape[0] and W3.shape[0] <= 8 and
            W2.shape[0] % 32 == 0 and Wg.shape[0] <= 4096 and B <= 32 and (8 if B <= 8 else 32) * W0.shape[0] <= 8192)


def seg_head(levels, B, Npts, global_block, seg_blocks):
    """DGCNNSeg's head on point-major `levels` (B * Npts, 192): global feature block (conv, BN, LeakyReLU) + the four
    segmentation blocks -> logits (B * Npts, classes).  See _SegHead."""
    gconv, gbn, gact = global_block.layers
    (c0, bn0, _), (c1, bn1, _), (c2, bn2, _) = (blk.layers for blk in seg_blocks[:3])
    c3 = seg_blocks[3].layers[0]
    bns = (gbn, bn0, bn1, bn2)
    steps = tuple(_bn_step(bn) for bn in bns)
    w = lambda conv: conv.weight.view(conv.out_channels, conv.in_channels)
    return _SegHead.apply(levels, B, Npts, float(gact.negative_slope), bns, steps, w(gconv), gbn.weight, gbn.bias, w(c0),
                          bn0.weight, bn0.bias, w(c1), bn1.weight, bn1.bias, w(c2), bn2.weight, bn2.bias, w(c3), c3.bias)


# ------------------------------------------------------------------ BatchNorm + LeakyReLU on (M, C) rows
class _BNAct(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, y, gamma, beta, rm, rv, training, momentum, eps, slope):
        y, gamma, beta = _f32c(y), _f32c(gamma), _f32c(beta)
        M, C = y.shape
        dev = y.device
        out = torch.empty_like(y)
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            invstd = torch.empty(C, dtype=torch.float32, device=dev)
            ws = _lib.workspace("fsg_bn_act", M, C, device=dev)
        else:
            (mean, invstd), ws = _bn_eval_stats(rm, rv, eps), None
        with torch.cuda.device(dev):
            _lib.call("fsg_bn_act_fwd_f32", _p(y), _p(gamma), _p(beta), _p(rm if training else None),
                      _p(rv if training else None), M, C, int(training), momentum, eps, slope, _p(out), _p(mean),
                      _p(invstd), _p(ws), _stream())
        ctx.save_for_backward(y, gamma, beta, mean, invstd)
        ctx.meta = (M, C, bool(training), slope)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        y, gamma, beta, mean, invstd = ctx.saved_tensors
        M, C, training, slope = ctx.meta
        g = _f32c(g)
        gy = torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        ws = _lib.workspace("fsg_bn_act", M, C, device=y.device)
        with torch.cuda.device(y.device):
            _lib.call("fsg_bn_act_bwd_f32", _p(g), _p(y), _p(gamma), _p(beta), _p(mean), _p(invstd), M, C, int(training),
                      slope, _p(gy), _p(dgamma), _p(dbeta), _p(ws), _stream())
        return gy, dgamma, dbeta, None, None, None, None, None, None


class _BNActMax(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, y, gamma, beta, rm, rv, training, momentum, eps, slope):
        y, gamma, beta = _f32c(y), _f32c(gamma), _f32c(beta)
        B, N, C = y.shape
        dev = y.device
        out = torch.empty(B, C, dtype=torch.float32, device=dev)
        ysel = torch.empty(B, C, dtype=torch.float32, device=dev)
        arg = torch.empty(B, C, dtype=torch.int32, device=dev)
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            invstd = torch.empty(C, dtype=torch.float32, device=dev)
        else:
            mean, invstd = _bn_eval_stats(rm, rv, eps)
        ws = _lib.workspace("fsg_bn_act_max", B, N, C, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_bn_act_max_fwd_f32", _p(y), _p(gamma), _p(beta), _p(rm if training else None),
                      _p(rv if training else None), B, N, C, int(training), momentum, eps, slope, _p(out), _p(ysel),
                      _p(arg), _p(mean), _p(invstd), _p(ws), _stream())
        ctx.save_for_backward(y, gamma, beta, mean, invstd, ysel, arg)
        ctx.meta = (B, N, C, bool(training), slope)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        y, gamma, beta, mean, invstd, ysel, arg = ctx.saved_tensors
        B, N, C, training, slope = ctx.meta
        g = _f32c(g)
        gy = torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        with torch.cuda.device(y.device):
            _lib.call("fsg_bn_act_max_bwd_f32", _p(g), _p(y), _p(ysel), _p(arg), _p(gamma), _p(beta), _p(mean), _p(invstd),
                      B, N, C, int(training), slope, _p(gy), _p(dgamma), _p(dbeta), _stream())
        return gy, dgamma, dbeta, None, None, None, None, None, None


def bn_act_max(y, bn, slope):
    """max over dim 1 of LeakyReLU(slope)(BatchNorm(y)) for y (B, N, C) -> (B, C), without the (B,N,C) activation."""
    _need_gpu(y)
    return _BNActMax.apply(y, *_bn_args(bn), float(slope))


class _BNActMaxAvg(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, y, gamma, beta, rm, rv, training, momentum, eps, slope):
        y, gamma, beta = _f32c(y), _f32c(gamma), _f32c(beta)
        B, N, C = y.shape
        dev = y.device
        out = torch.empty(B, 2 * C, dtype=torch.float32, device=dev)
        arg = torch.empty(B, C, dtype=torch.int32, device=dev)
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            invstd = torch.empty(C, dtype=torch.float32, device=dev)
        else:
            mean, invstd = _bn_eval_stats(rm, rv, eps)
        ws = _lib.workspace("fsg_bn_act_maxavg", B, N, C, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_bn_act_maxavg_fwd_f32", _p(y), _p(gamma), _p(beta), _p(rm if training else None),
                      _p(rv if training else None), B, N, C, int(training), momentum, eps, slope, _p(out), _p(arg),
                      _p(mean), _p(invstd), _p(ws), _stream())
        ctx.save_for_backward(y, gamma, beta, mean, invstd, arg)
        ctx.meta = (B, N, C, bool(training), slope)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        y, gamma, beta, mean, invstd, arg = ctx.saved_tensors
        B, N, C, training, slope = ctx.meta
        g = _f32c(g)
        gy = torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        ws = _lib.workspace("fsg_bn_act_maxavg", B, N, C, device=y.device)
        with torch.cuda.device(y.device):
            _lib.call("fsg_bn_act_maxavg_bwd_f32", _p(g), _p(y), _p(arg), _p(gamma), _p(beta), _p(mean), _p(invstd),
                      B, N, C, int(training), slope, _p(gy), _p(dgamma), _p(dbeta), _p(ws), _stream())
        return gy, dgamma, dbeta, None, None, None, None, None, None


def bn_act_maxavg(y, bn, slope):
    """cat(max, mean) over dim 1 of LeakyReLU(slope)(BatchNorm(y)) for y (B, N, C) -> (B, 2C), without the (B,N,C)
    activation (models/dgcnn_opensrc.py:158-164)."""
    _need_gpu(y)
    return _BNActMaxAvg.apply(y, *_bn_args(bn), float(slope))


def bn_act_supported(y, bn):
    return y.is_cuda and y.dim() == 2 and y.shape[1] % 64 == 0 and bn.affine


def bn_act(y, bn, slope):
    """LeakyReLU(slope)(BatchNorm1d(y)) for point-major rows y (M, C): one fused HIP stage (slope 1: BN only)."""
    _need_gpu(y)
    return _BNAct.apply(y, *_bn_args(bn), float(slope))


# ------------------------------------------------------------------ BatchNorm (+ residual) (+ ReLU) over packed rows
BN_ROWS_WIDTHS = (32, 64, 128, 256, 512)


class _BNRows(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, res, gamma, beta, rm, rv, training, momentum, eps, relu):
        M, C = x.shape
        dev = x.device
        out = torch.empty_like(x)
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            rstd = torch.empty(C, dtype=torch.float32, device=dev)
            ws = _lib.workspace("fsg_bn_rows", M, C, device=dev)
        else:
            (mean, rstd), ws = _bn_eval_stats(rm, rv, eps), None
        with torch.cuda.device(dev):
            _lib.call("fsg_bn_rows_fwd_f32", _p(x), _p(res), _p(gamma), _p(beta), _p(rm if training else None),
                      _p(rv if training else None), M, C, int(training), momentum, eps, int(relu), _p(out), _p(mean),
                      _p(rstd), _p(ws), _stream())
        ctx.save_for_backward(x, out, gamma, mean, rstd)
        ctx.meta = (M, C, bool(training), bool(relu), res is not None)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, out, gamma, mean, rstd = ctx.saved_tensors
        M, C, training, relu, has_res = ctx.meta
        g = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if has_res else None
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = _lib.workspace("fsg_bn_rows", M, C, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("fsg_bn_rows_bwd_f32", _p(g), _p(x), _p(out), _p(gamma), _p(mean), _p(rstd), M, C, int(training),
                      int(relu), _p(gx), _p(gres), _p(dgamma), _p(dbeta), _p(ws), _stream())
        return gx, gres, dgamma, dbeta, None, None, None, None, None, None


def bn_rows_supported(x, bn):
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] in BN_ROWS_WIDTHS and x.shape[0] > 0
            and bn.affine and (bn.training or bn.running_mean is not None))


def bn_rows(x, bn, relu=True, residual=None):
    """[relu]( BatchNorm1d(x) [+ residual] ) for packed point rows x (M, C): one fused HIP stage (3 launches forward,
    3 backward) instead of ATen's 4-5 + 3-5.  Same running-statistics semantics as torch.nn.BatchNorm1d."""
    _need_gpu(x)
    bn_args = _bn_args(bn)
    if x.dtype != torch.float32:                  # the kernels read fp32 rows (the other fused stages widen in _f32c)
        x = x.float()
    x = x if x.is_contiguous() else x.contiguous()
    if residual is not None and (residual.dtype != torch.float32 or not residual.is_contiguous()):
        residual = residual.float().contiguous()
    return _BNRows.apply(x, residual, *bn_args, relu)


# ------------------------------------------------------------------ Chamfer (losses/chamfer_loss.py:19)
class _ChamferNN(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, y):
        xc, yc = _f32c(x), _f32c(y)
        B, N, _ = xc.shape
        M = yc.shape[1]
        d = torch.empty(B, N, dtype=torch.float32, device=x.device)
        a = torch.empty(B, N, dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("fsg_chamfer_nn_f32", _p(xc), _p(yc), B, N, M, _p(d), _p(a), _stream())
        ctx.save_for_backward(xc, yc, a)
        ctx.mark_non_differentiable(a)
        return d, a

    @staticmethod
    @_amp_bwd
    def backward(ctx, gd, _ga):
        xc, yc, a = ctx.saved_tensors
        B, N, _ = xc.shape
        M = yc.shape[1]
        gx, gy = torch.zeros_like(xc), torch.zeros_like(yc)
        ws = None
        if deterministic():
            ws = _lib.workspace("fsg_chamfer_nn_bwd", B, N, M, device=xc.device)
        with torch.cuda.device(xc.device):
            _lib.call("fsg_chamfer_nn_bwd_f32", _p(xc), _p(yc), _p(a), _p(_f32c(gd)), B, N, M, _p(gx), _p(gy), _p(ws),
                      _stream())
        return gx, gy


def chamfer_nn(x, y):
    """x (B,N,3), y (B,M,3) -> (min squared distance (B,N), argmin (B,N) int32); differentiable in x, y."""
    _need_gpu(x, y)
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
        raise ValueError(f"expected (B,N,3) and (B,M,3), got {tuple(x.shape)} and {tuple(y.shape)}")
    return _ChamferNN.apply(x, y)


# ------------------------------------------------------------------ point-to-mesh distance (metrics.py:11-25)
_faces_checked = {}   # (storage, data_ptr, version, shape, strides, dtype) -> (weak storage reference, lowest, highest index)


def _faces_range(faces):
    """(lowest, highest) index of a faces tensor: one reduction and one synchronisation per tensor, remembered by storage,
    address and version counter (an in-place write bumps the version, so a modified list is looked at again).  The entry
    holds a weak reference to the storage: an address alone says nothing once the tensor is gone and the allocator has handed
    its memory to another one."""
    from torch.multiprocessing.reductions import StorageWeakRef
    storage = faces.untyped_storage()
    key = (storage._cdata, faces.data_ptr(), faces._version, tuple(faces.shape), faces.stride(), faces.dtype)
    got = _faces_checked.get(key)
    if got is None or got[0].expired():
        for k in [k for k, v in _faces_checked.items() if v[0].expired()]:
            del _faces_checked[k]
        if len(_faces_checked) >= 64:
            _faces_checked.clear()
        lo, hi = torch.aminmax(faces)
        got = _faces_checked[key] = (StorageWeakRef(storage), int(lo), int(hi))
    return got[1], got[2]


def point_mesh_distance(points, verts, faces, return_face=False, return_closest=False, validate=True):
    """Unsigned Euclidean distance from every point to a triangle mesh (fsg_point_mesh_dist_f32; the square root is torch's).

    points (B,P,3), verts (B,V,3), faces (F,3) shared by all meshes or (B,F,3) -> dist (B,P) fp32
    [, face (B,P) int32: a face that attains it, the lowest index on ties][, closest (B,P,3): the closest point on it].
    Faces without area are legal (distance to their longest edge, or to the point).  `validate` checks the face indices
    against V once per faces tensor; the kernel itself does not.  P == 0 gives empty results, F == 0 (or V == 0) NaN
    distances, face -1 and NaN closest points; no kernel is launched then.

    An evaluation primitive, NOT differentiable: it runs under torch.no_grad and its outputs never require grad.  A
    point-to-surface loss (the gradient with respect to points and vertices) is not part of this package yet."""
    _need_gpu(points, verts, faces)
    if (points.dim() != 3 or verts.dim() != 3 or points.shape[2] != 3 or verts.shape[2] != 3 or points.shape[0] != verts.shape[0]
            or faces.dim() not in (2, 3) or faces.shape[-1] != 3 or (faces.dim() == 3 and faces.shape[0] != verts.shape[0])):
        raise ValueError(f"expected points (B,P,3), verts (B,V,3) and faces (F,3) or (B,F,3), got {tuple(points.shape)}, "
                         f"{tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError(f"faces must hold integer vertex indices, got {faces.dtype}")
    with torch.no_grad():
        pc, vc = _f32c(points), _f32c(verts)
        B, P, _ = pc.shape
        V, F = vc.shape[1], faces.shape[-2]
        dev = pc.device
        if P == 0 or F == 0 or V == 0 or B == 0:
            out = [torch.full((B, P), float("nan"), dtype=torch.float32, device=dev)]
            if return_face:
                out.append(torch.full((B, P), -1, dtype=torch.int32, device=dev))
            if return_closest:
                out.append(torch.full((B, P, 3), float("nan"), dtype=torch.float32, device=dev))
            return out[0] if len(out) == 1 else tuple(out)
        if validate:
            lo, hi = _faces_range(faces)
            if lo < 0 or hi >= V:
                raise ValueError(f"face indices span [{lo}, {hi}] but the mesh has {V} vertices")
        fc = faces.detach().to(torch.int32).contiguous()
        d2 = torch.empty(B, P, dtype=torch.float32, device=dev)
        face = torch.empty(B, P, dtype=torch.int32, device=dev) if return_face else None
        closest = torch.empty(B, P, 3, dtype=torch.float32, device=dev) if return_closest else None
        with torch.cuda.device(dev):
            _lib.call("fsg_point_mesh_dist_f32", _p(pc), _p(vc), _p(fc), B, P, V, F, B if fc.dim() == 3 else 1, _p(d2), _p(face),
                      _p(closest), _stream())
        out = [d2.sqrt_()] + [t for t in (face, closest) if t is not None]
    return out[0] if len(out) == 1 else tuple(out)


# ------------------------------------------------------------------ meshes -> voxel label maps (csrc/voxelize.hip)
def _pack_meshes(who, verts, faces, shape, spacing, validate):
    """the meshes of one call as one vertex list, one face list (indices shifted) and the mesh number of every face; meshes
    without vertices or faces are left out but keep their number.  -> (verts, faces, labels) or None if nothing is left,
    shape and spacing as tuples, the device"""
    verts, faces = ([x] if torch.is_tensor(x) else list(x) for x in (verts, faces))
    if len(verts) != len(faces) or not verts:
        raise ValueError(f"{who}: expected as many vertex tensors as face tensors and at least one, got {len(verts)} and {len(faces)}")
    _need_gpu(*verts, *faces)
    shape, spacing = tuple(int(n) for n in shape), tuple(float(s) for s in spacing)
    if len(shape) != 3 or len(spacing) != 3:
        raise ValueError(f"{who}: expected a 3-D shape and one spacing per axis, got {shape} and {spacing}")
    dev = verts[0].device
    vs, fs, ls, base = [], [], [], 0
    for m, (v, f) in enumerate(zip(verts, faces)):
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"{who}: mesh {m}: expected verts (V,3) and faces (F,3), got {tuple(v.shape)} and {tuple(f.shape)}")
        if f.is_floating_point() or f.dtype == torch.bool:
            raise ValueError(f"{who}: mesh {m}: faces must hold integer vertex indices, got {f.dtype}")
        if v.shape[0] == 0 or f.shape[0] == 0:
            continue
        if validate:
            lo, hi = _faces_range(f)
            if lo < 0 or hi >= v.shape[0]:
                raise ValueError(f"{who}: mesh {m}: face indices span [{lo}, {hi}] but the mesh has {v.shape[0]} vertices")
            if not bool(torch.isfinite(v).all()):
                raise ValueError(f"{who}: mesh {m} has a non-finite vertex")
        vs.append(_f32c(v))
        fs.append(f.detach().to(torch.int32) + base)
        ls.append(torch.full((f.shape[0],), m, dtype=torch.int32, device=dev))
        base += v.shape[0]
    packed = (torch.cat(vs), torch.cat(fs).contiguous(), torch.cat(ls)) if vs else None
    return packed, shape, spacing, dev


def mesh_labelmap_dist(verts, faces, shape, spacing, dist_threshold=1.0, mask=None, validate=True):
    """Label map of the voxels within `dist_threshold` of a set of triangle meshes (fsg_mesh_labelmap_dist_f32).

    verts: list of (V_m,3), faces: list of (F_m,3) integer tensors on the GPU (one tensor each for a single mesh); vertex
    coordinates in the axis order of the volume, in the units of `spacing` (s0, s1, s2); voxel (i0,i1,i2) has the centre
    (i0 s0, i1 s1, i2 s2).  -> int64 tensor of `shape`: 1 + m for the mesh m of smallest distance if that distance is
    <= dist_threshold and `mask` (bool, `shape`; None = everywhere) is set, else 0; the lowest m on an exact tie.  A mesh
    without vertices or faces takes part in nothing, the others keep their numbers.  Distances are those of
    `point_mesh_distance`; faces without area are legal.  Bitwise reproducible.

    `validate` checks the face indices against V (once per faces tensor) and that the vertices are finite, and raises
    ValueError before anything is launched; the kernel clips in float and never forms an index from a coordinate outside
    the volume, but does not check face indices.  Not differentiable."""
    packed, shape, spacing, dev = _pack_meshes("mesh_labelmap_dist", verts, faces, shape, spacing, validate)
    if mask is not None:
        _need_gpu(mask)
        if tuple(mask.shape) != shape:
            raise ValueError(f"mesh_labelmap_dist: mask of shape {tuple(mask.shape)} for a volume of {shape}")
        mask = (mask.detach() != 0).contiguous()
    if packed is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    v, f, lab = packed
    out = torch.empty(shape, dtype=torch.int64, device=dev)
    keys = torch.empty(shape, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fsg_mesh_labelmap_dist_f32", _p(v), _p(f), _p(lab), v.shape[0], f.shape[0], *shape, *spacing,
                  float(dist_threshold), _p(mask), _p(keys), _p(out), _stream())
    return out


def mesh_labelmap_cover(verts, faces, shape, spacing, validate=True):
    """Label map of the cells that the surface of a set of triangle meshes passes through (fsg_mesh_labelmap_cover_f32): what
    scattering floor(sample / spacing) of surface samples tends to as their number grows.

    Arguments as for `mesh_labelmap_dist`.  Cell (i0,i1,i2) is the box [i s, (i + 1) s) per axis.  -> int64 tensor of `shape`:
    the highest 1 + m among the meshes with a triangle that intersects the cell, 0 if none; parts of a mesh outside the
    volume are dropped.  A face without area counts as its longest edge (or its point).  Bitwise reproducible."""
    packed, shape, spacing, dev = _pack_meshes("mesh_labelmap_cover", verts, faces, shape, spacing, validate)
    if packed is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    v, f, lab = packed
    out = torch.empty(shape, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fsg_mesh_labelmap_cover_f32", _p(v), _p(f), _p(lab), v.shape[0], f.shape[0], *shape, *spacing, _p(out), _stream())
    return out


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
        with torch.cuda.device(w.device):
            _lib.call("fsg_ssm_decode_fwd_f32", _p(wc), _p(mc), _p(ec), _p(vc), _p(sc), _p(tc), B, P, M, _p(out), _stream())
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
        with torch.cuda.device(dev):
            _lib.call("fsg_ssm_decode_bwd_f32", _p(_f32c(g)), _p(wc), _p(mc), _p(ec), _p(vc), _p(sc), B, P, M, _p(dw), _p(dv),
                      _p(ds), _p(dt), _p(ws), ws.numel(), _stream())
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
        with torch.cuda.device(dev):
            _lib.call("fsg_cpd_estep_f32", _p(xc), 3 * N if xc.dim() == 3 else 0, _p(yc), _p(sc), float(w), B, N, M, _p(P1),
                      _p(Pt1), _p(PX), _p(Np), _p(ws), ws.numel(), _stream())
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
        with torch.cuda.device(dev):
            _lib.call("fsg_kmeans_prepare_f32", _p(points), _p(centroids), B, n, K, float(tol), _p(self.ws), self.ws.numel(),
                      _stream())

    def launch(self, entry):
        B, n, K = self.dims
        with torch.cuda.device(self.dev):
            _lib.call(entry, _p(self.points), _p(self.centroids), _p(self.labels), B, n, K, _p(self.ws), self.ws.numel(),
                      _p(self.counts), _p(self.stats), _p(self.info), _stream())


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
        with torch.cuda.device(cc.device):
            _lib.call("fsg_tps_system_f64", _p(cc), B, n, float(lambd), _p(A), _stream())
    return A[0] if squeeze else A


def tps_fit(control, values, lambd=0., fit_batch=32):
    """TPS.fit for a batch: control (B,n,3), values (B,n,C) (or (n,3), (n,C)) -> theta (B,n+4,C) fp64, the n spline weights and
    the four affine rows.  The systems come from `tps_system`, the solve is torch's batched fp64 linalg.solve, `fit_batch`
    systems at a time (100 systems of 1028^2 in fp64 are 0.85 GB).  n >= 4 points not in one plane (or lambd > 0 with
    distinct points) make the system regular; a singular one raises as linalg.solve does."""
    c, squeeze = _tps_points(control, "control", "tps_fit")
    if not torch.is_tensor(values) or not values.is_floating_point() or values.dim() != control.dim() \
            or values.shape[:-1] != control.shape[:-1]:
        got = f"{tuple(values.shape)} {values.dtype}" if torch.is_tensor(values) else type(values).__name__
        raise ValueError(f"tps_fit: values must be floating-point {tuple(control.shape[:-1])} + (C,), got {got}")
    v = values[None] if squeeze else values
    if not 1 <= v.shape[2] <= TPS_MAX_CHANNELS:
        raise ValueError(f"tps_fit: C={v.shape[2]} channels, the kernels serve 1 <= C <= {TPS_MAX_CHANNELS}")
    if isinstance(fit_batch, bool) or not isinstance(fit_batch, int) or fit_batch < 1:
        raise ValueError(f"tps_fit: fit_batch must be a positive integer, got {fit_batch!r}")
    _need_gpu(c, v)
    _tps_same_device("tps_fit", c, v)
    B, n, C = v.shape
    with torch.no_grad():
        theta = torch.empty(B, n + 4, C, dtype=torch.float64, device=c.device)
        for b0 in range(0, B, fit_batch):
            A = tps_system(c[b0:b0 + fit_batch], lambd)
            rhs = torch.zeros(A.shape[0], n + 4, C, dtype=torch.float64, device=c.device)
            rhs[:, :n] = v[b0:b0 + fit_batch]
            theta[b0:b0 + fit_batch] = torch.linalg.solve(A, rhs)
    return theta[0] if squeeze else theta


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
        with torch.cuda.device(cc.device):
            _lib.call("fsg_tps_eval_f32", _p(qc), _p(cc), _p(tc), B, Q, n, C, *lattice, _p(out), _stream())
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
        with torch.cuda.device(cc.device):
            _lib.call("fsg_tps_grid_sample_f32", _p(gc), _p(cc), _p(tc), B, Q, n, C, *size, *coarse, _p(out), _stream())
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
        with torch.cuda.device(dev):
            _lib.call("fsg_sample_elimination_f32", _p(pc), _p(radii), B, M, n_keep, _p(keep), _p(order), _p(ws), ws.numel(),
                      _stream())
        out = [keep.long()] + ([order.long()] if return_order else [])
    if squeeze:
        out = [t[0] for t in out]
    return tuple(out) if return_order else out[0]


# ------------------------------------------------------------------ segmentation loss (losses/nnu_loss.py:6-19)
class _NNULoss(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, logits, target, class_weights, w_ce, w_dice, smooth):
        B, C, N = logits.shape
        dev = logits.device
        vals = torch.empty(4, dtype=torch.float32, device=dev)
        need_grad = ctx.needs_input_grad[0]
        grad = torch.empty_like(logits) if need_grad else None      # keeps the (possibly point-major) strides
        if grad is not None and grad.stride() != logits.stride():
            grad = torch.empty_strided(logits.shape, logits.stride(), dtype=torch.float32, device=dev)
        ws = _lib.workspace("fsg_nnu_loss", C, device=dev)
        gs = grad.stride() if grad is not None else (0, 0, 0)
        with torch.cuda.device(dev):
            _lib.call("fsg_nnu_loss_f32", _p(logits), logits.stride(0), logits.stride(1), logits.stride(2), _p(target),
                      _p(class_weights) if class_weights is not None else None, B, C, N, float(w_ce), float(w_dice),
                      float(smooth), _p(vals), _p(grad) if grad is not None else None, gs[0], gs[1], gs[2], _p(ws),
                      _stream())
        ctx.grad = grad
        total, ce, gdl = vals[0], vals[1], vals[2]
        ctx.mark_non_differentiable(ce, gdl)
        ctx.set_materialize_grads(False)      # no zero tensors for the two logging outputs
        return total, ce, gdl

    @staticmethod
    @_amp_bwd
    def backward(ctx, g, _gce, _ggdl):
        grad, ctx.grad = ctx.grad, None
        if g is None:
            return None, None, None, None, None, None
        return grad * g, None, None, None, None, None


def nnu_loss(logits, target, class_weights=None, w_ce=1.0, w_dice=1.0, smooth=1.0):
    """CrossEntropyLoss(class_weights) + generalised Dice (softmax, batch_dice) of logits (B,C,N) against labels (B,N).

    Returns 0-d tensors (w_ce*ce + w_dice*gdl, ce, gdl); the first is differentiable in `logits` (any strides), the
    other two are for logging.  The gradient is produced by the same two launches that evaluate the loss."""
    _need_gpu(logits, target)
    if logits.dim() != 3 or target.shape != (logits.shape[0], logits.shape[2]):
        raise ValueError(f"expected logits (B,C,N) and labels (B,N), got {tuple(logits.shape)} and {tuple(target.shape)}")
    if not 2 <= logits.shape[1] <= 32:
        raise ValueError(f"number of classes must be in [2, 32], got {logits.shape[1]}")
    if logits.dtype != torch.float32:
        logits = logits.float()
    target = target.to(torch.int64).contiguous()
    if class_weights is not None:
        if class_weights.numel() != logits.shape[1]:
            raise ValueError("class_weights must have one entry per class")
        class_weights = _f32c(class_weights.to(logits.device))
    return _NNULoss.apply(logits, target, class_weights, w_ce, w_dice, smooth)


# ------------------------------------------------------------------ packed clouds (pointops.py)
def knn_segment(nsample, xyz, new_xyz, offset, new_offset):
    """-> idx (m,nsample) int32, dist2 (m,nsample) squared distances."""
    _need_gpu(xyz, new_xyz, offset, new_offset)
    xyz, new_xyz = _f32c(xyz), _f32c(new_xyz)
    offset, new_offset = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    m = new_xyz.shape[0]
    idx = torch.empty(m, nsample, dtype=torch.int32, device=xyz.device)
    d2 = torch.empty(m, nsample, dtype=torch.float32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.call("fsg_knn_segment_f32", _p(xyz), _p(new_xyz), _p(offset), _p(new_offset), offset.shape[0],
                  xyz.shape[0], m, nsample, _p(idx), _p(d2), _stream())
    return idx, d2


def fps(xyz, offset, new_offset, m):
    """m = total number of samples (new_offset[-1], known on the host) -> idx (m) int32."""
    _need_gpu(xyz, offset, new_offset)
    xyz = _f32c(xyz)
    offset, new_offset = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    n = xyz.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=xyz.device)     # every entry is written (empty segments: zeros, by the kernel)
    tmp = torch.empty(n, dtype=torch.float32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.call("fsg_fps_f32", _p(xyz), _p(offset), _p(new_offset), offset.shape[0], n, _p(tmp), _p(idx), _stream())
    return idx


# ------------------------------------------------------------------ DSEG-AE glue (csrc/dseg_ae.hip)
PARTITION_MAX_LABELS = _lib.PARTITION_MAX_LABELS


def label_partition(labels, x, num_labels, first_label=1):
    """labels (B, N) uint8 / int32 / int64, x (B, C, N) with the coordinates in its first three channels -> the points of the
    objects first_label .. first_label + num_labels - 1 as packed segments, one per (item, object) in that order:
    counts (B, num_labels) int32, offset (B * num_labels) int32 (the end of every segment), xyz (B * N, 3) fp32 and
    src (B * N) int32 (the point's index inside its item), of which the first offset[-1] rows are filled and the rest are
    zero.  Inside a segment the points keep their order.  Any other label is dropped.  Nothing is read on the host."""
    if labels.dim() != 2 or x.dim() != 3 or x.shape[0] != labels.shape[0] or x.shape[2] != labels.shape[1] or x.shape[1] < 3:
        raise ValueError(f"label_partition: labels (B, N) and x (B, C >= 3, N) expected, got {tuple(labels.shape)} and {tuple(x.shape)}")
    if labels.dtype not in _LABEL_KINDS:
        raise TypeError(f"label_partition: labels must be uint8, int32 or int64, got {labels.dtype}")
    L = int(num_labels)
    if not 1 <= L <= PARTITION_MAX_LABELS:
        raise ValueError(f"label_partition: num_labels must be in 1..{PARTITION_MAX_LABELS}, got {num_labels}")
    B, N = labels.shape
    if B == 0 or N == 0 or B * N >= 2 ** 31:
        raise ValueError(f"label_partition: {B} clouds of {N} points (1 <= B * N < 2^31)")
    _need_gpu(labels, x)
    labels, x = labels.contiguous(), _f32c(x)
    dev = x.device
    counts = torch.empty(B, L, dtype=torch.int32, device=dev)
    offset = torch.empty(B * L, dtype=torch.int32, device=dev)
    xyz = torch.zeros(B * N, 3, dtype=torch.float32, device=dev)
    src = torch.zeros(B * N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _lib.workspace("fsg_label_partition", B, N, L, device=dev)
        _lib.call("fsg_label_partition", _p(labels), _LABEL_KINDS[labels.dtype], _p(x), B, x.shape[1], N, int(first_label), L,
                  _p(counts), _p(offset), _p(xyz), _p(src), _p(ws), ws.numel(), _stream())
    return counts, offset, xyz, src


def segment_jitter_extend(xyz, offset, target, src_idx, direction, z, nn_d2=None):
    """`random_extend_points` of dseg_ae_regularization.py for G packed segments in one launch.  xyz (n, 3) with offset (G)
    HOST-known segment ends (a list, or a tensor that is read on the host); every segment grows to max(its length, target) --
    target a number or one per segment.  The caller's draws cover the P padded rows, packed in segment order: src_idx (P)
    the source row inside the segment, direction (P, 3), z (P).  nn_d2 (n): squared distance to the nearest OTHER point of
    the segment; by default column 1 of `knn_segment(2, xyz, xyz, offset, offset)`.
    -> out (n_new, 3), new_offset (G) int32 on the device, stats (G, 2) = mean and unbiased std of the nearest distances
    (0, 0 for fewer than two points).  A padded row is xyz[src] + direction / |direction| * (z * std + mean)."""
    _need_gpu(xyz, src_idx, direction, z, nn_d2)
    ends = [int(v) for v in (offset.tolist() if torch.is_tensor(offset) else offset)]
    G = len(ends)
    lens = [e - s for s, e in zip([0] + ends[:-1], ends)]
    tg = [int(v) for v in (target.tolist() if torch.is_tensor(target) else target)] if hasattr(target, "__len__") else [int(target)] * G
    if xyz.dim() != 2 or xyz.shape[1] != 3 or G == 0 or len(tg) != G or min(lens) < 0 or ends[-1] != xyz.shape[0] or xyz.shape[0] == 0:
        raise ValueError(f"segment_jitter_extend: xyz {tuple(xyz.shape)} with segment ends {ends} and {len(tg)} targets")
    new_lens = [max(n, t) for n, t in zip(lens, tg)]
    n, n_new = ends[-1], sum(new_lens)
    P = n_new - n
    if src_idx.numel() != P or tuple(direction.shape) != (P, 3) or z.numel() != P:
        raise ValueError(f"segment_jitter_extend: {P} padded rows, draws of {src_idx.numel()}, {tuple(direction.shape)}, {z.numel()}")
    dev = xyz.device
    xyz = _f32c(xyz)
    off = torch.tensor(ends, dtype=torch.int32).to(dev)
    new_off = torch.tensor(new_lens, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
    if nn_d2 is None:
        nn_d2 = knn_segment(2, xyz, xyz, off, off)[1][:, 1]
    if nn_d2.shape != (n,):
        raise ValueError(f"segment_jitter_extend: nn_d2 {tuple(nn_d2.shape)} for {n} points")
    nn_d2 = _f32c(nn_d2)
    src_idx, direction, z = src_idx.to(torch.int32).contiguous(), _f32c(direction), _f32c(z).reshape(-1)
    out = torch.empty(n_new, 3, dtype=torch.float32, device=dev)
    stats = torch.empty(G, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fsg_segment_jitter_extend_f32", _p(xyz), _p(off), _p(nn_d2), _p(new_off), _p(src_idx), _p(direction), _p(z), G, n,
                  n_new, _p(out), _p(stats), _stream())
    return out, new_off, stats


def fps_start(xyz, offset, new_offset, m, start=None):
    """`fps` with a first sample per segment: start (b) = its index INSIDE the segment (None: 0, and then the result equals
    `fps`'s bit for bit).  One workgroup of 1024 threads per segment; segments of up to 16 384 points are sampled from
    registers.  m = total number of samples (new_offset[-1], known on the host) -> idx (m) int32 into xyz."""
    _need_gpu(xyz, offset, new_offset, start)
    xyz = _f32c(xyz)
    offset, new_offset = offset.to(torch.int32).contiguous(), new_offset.to(torch.int32).contiguous()
    if start is not None:
        if start.shape != offset.shape:
            raise ValueError(f"fps_start: start {tuple(start.shape)} for {offset.shape[0]} segments")
        start = start.to(torch.int32).contiguous()
    n = xyz.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=xyz.device)     # every entry is written (empty segments: zeros, by the kernel)
    tmp = torch.empty(n, dtype=torch.float32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.call("fsg_fps_start_f32", _p(xyz), _p(offset), _p(new_offset), _p(start), offset.shape[0], n, _p(tmp), _p(idx),
                  _stream())
    return idx


# ------------------------------------------------------------------ point-cloud normals (csrc/pcl_normals.hip)
def _neighborhood_size(neighborhood_size):
    K = int(neighborhood_size)
    if not 2 <= K <= _lib.PCL_NORMALS_MAX_K:
        raise ValueError(f"neighborhood_size must be in 2..{_lib.PCL_NORMALS_MAX_K}, got {neighborhood_size}")
    return K


def _check_neighbours(idx, off, n, K):
    """the host-side look at a caller's neighbour lists (one synchronisation): the offsets end at n and do not decrease, and
    every column the kernel reads (the first k_s of a row) names a point of the row's own segment"""
    rows = torch.arange(n, device=idx.device)
    seg = torch.searchsorted(off, rows.to(torch.int32), right=True).clamp_(max=off.shape[0] - 1)
    en = off[seg].long()
    st = torch.where(seg > 0, off[(seg - 1).clamp_(min=0)].long(), torch.zeros_like(en))
    ks = (en - st - 1).clamp_(min=1, max=K)
    read = torch.arange(K, device=idx.device)[None] < ks[:, None]
    i = idx.long()
    bad_idx = (read & ((i < st[:, None]) | (i >= en[:, None]))).any()
    bad_off = (off[-1] != n) | (off[0] < 0) | (off[1:] < off[:-1]).any()
    bad_idx, bad_off = torch.stack([bad_idx, bad_off]).tolist()
    if bad_off:
        raise ValueError(f"offset must be non-decreasing cumulative segment ends finishing at n = {n}")
    if bad_idx:
        raise ValueError("idx holds an index outside its row's segment (or outside the cloud) in a column that is read")


def _pcl_normals_raw(xyz, off, K, disambiguate, idx, want_frames):
    """xyz (n, 3) fp32 contiguous, off (b) int32, idx (n, K) int32 -> normals (n, 3), curvatures (n, 3), frames (n, 3, 3) | None"""
    n = xyz.shape[0]
    normals = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
    curv = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
    frames = torch.empty(n, 3, 3, dtype=torch.float32, device=xyz.device) if want_frames else None
    with torch.cuda.device(xyz.device):
        _lib.call("fsg_pcl_normals_f32", _p(xyz), _p(idx), _p(off), off.shape[0], n, K, int(bool(disambiguate)), _p(normals),
                  _p(curv), _p(frames), _stream())
    return normals, curv, frames


def _pcl_packed(xyz, offset, neighborhood_size, disambiguate_directions, idx, validate, want_frames):
    K = _neighborhood_size(neighborhood_size)
    if not torch.is_tensor(xyz) or not xyz.is_floating_point() or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"expected packed points xyz (n, 3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if not torch.is_tensor(offset) or offset.is_floating_point() or offset.dim() != 1 or offset.shape[0] < 1:
        raise ValueError("offset must be a 1-D integer tensor of cumulative segment ends")
    _need_gpu(xyz, offset, idx)
    with torch.no_grad():
        x, off = _f32c(xyz), offset.to(torch.int32).contiguous()
        n = x.shape[0]
        if idx is None:
            idx = knn_segment(K, x, x, off, off)[0] if n else torch.empty(0, K, dtype=torch.int32, device=x.device)
        else:
            if not torch.is_tensor(idx) or idx.is_floating_point() or idx.dtype == torch.bool or tuple(idx.shape) != (n, K):
                raise ValueError(f"idx must be an integer tensor of shape ({n}, {K}): the first neighborhood_size columns of "
                                 f"knn_segment's lists")
            idx = idx.to(torch.int32).contiguous()
            if validate and n:
                _check_neighbours(idx, off, n, K)
        return _pcl_normals_raw(x, off, K, disambiguate_directions, idx, want_frames)


def pointcloud_frames_packed(xyz, offset, neighborhood_size, disambiguate_directions=True, idx=None, validate=True):
    """The local PCA frame of every point of a packed cloud (fsg_pcl_normals_f32): xyz (n, 3), offset (b,) cumulative segment
    ends -> curvatures (n, 3), the eigenvalues of the neighbourhood covariance in ascending order, and frames (n, 3, 3) whose
    COLUMNS are (normal, y, z): the eigenvector of the smallest eigenvalue, z x normal, the eigenvector of the largest.

    Per point: the k nearest points of its own segment, itself included; C = mean of (x_j - mean)(x_j - mean)^T over them.  A
    segment of n_s points uses k_s = min(neighborhood_size, n_s - 1) (at least 1): a short segment gets a smaller neighbourhood
    instead of an error.  With disambiguate_directions a vector v is negated when fewer than half of the k neighbours have
    v . (x_j - p) > 0 (applied to the normal and to z); on a convex surface this points the normals INWARDS, as pytorch3d's
    rule does.  Parity with pytorch3d is unpinned (restated, not compared).

    idx (n, neighborhood_size): neighbour lists in knn_segment's layout (ascending distance, self first, indices into xyz);
    without it knn_segment runs (queries = the points).  Only the first k_s columns of a row are read.  validate=True checks a
    given idx (and the offsets) on the host, one synchronisation: an index outside the row's segment raises ValueError; with
    validate=False a bad index is clamped into the cloud by the kernel and gives a wrong frame, not a fault.
    neighborhood_size outside 2..64 raises ValueError.  No autograd: the outputs are constants (detached), as the reference
    uses them.  Deterministic: the same input gives the same bits."""
    _, curv, frames = _pcl_packed(xyz, offset, neighborhood_size, disambiguate_directions, idx, validate, True)
    return curv, frames


def _dense_cloud(pointclouds, neighborhood_size):
    K = _neighborhood_size(neighborhood_size)
    if not torch.is_tensor(pointclouds) or pointclouds.dim() != 3 or pointclouds.shape[2] != 3:
        raise ValueError(f"expected pointclouds (B, N, 3), got "
                         f"{tuple(pointclouds.shape) if torch.is_tensor(pointclouds) else type(pointclouds).__name__}")
    B, N, _ = pointclouds.shape
    if K >= N:
        raise ValueError(f"neighborhood_size ({K}) must be smaller than the number of points per cloud ({N})")
    _need_gpu(pointclouds)
    offset = torch.arange(1, B + 1, dtype=torch.int32, device=pointclouds.device) * N
    return K, B, N, offset


def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=50, disambiguate_directions=True):
    """pytorch3d.ops.estimate_pointcloud_local_coord_frames for a (B, N, 3) tensor -> curvatures (B, N, 3), local_coord_frames
    (B, N, 3, 3); see pointcloud_frames_packed (every cloud is one segment).  2 <= neighborhood_size <= 64 and < N."""
    K, B, N, offset = _dense_cloud(pointclouds, neighborhood_size)
    _, curv, frames = _pcl_packed(pointclouds.reshape(B * N, 3), offset, K, disambiguate_directions, None, False, True)
    return curv.view(B, N, 3), frames.view(B, N, 3, 3)


def estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True):
    """pytorch3d.ops.estimate_pointcloud_normals for a (B, N, 3) tensor -> normals (B, N, 3), the first column of the frames of
    estimate_pointcloud_local_coord_frames (the same bits).  Constants: no gradient reaches the points."""
    K, B, N, offset = _dense_cloud(pointclouds, neighborhood_size)
    normals, _, _ = _pcl_packed(pointclouds.reshape(B * N, 3), offset, K, disambiguate_directions, None, False, False)
    return normals.view(B, N, 3)


# ------------------------------------------------------------------ zeroed scratch of a backward pass, one fill
class ZeroArena:
    """Backward kernels that accumulate with atomics (grouping, interpolation, the attention layer's dk / dv / dp) need zeroed
    buffers: 30 fill launches per PointTransformer step.  Inside `zero_arena()` the forward of each such Function RESERVES its
    size; the first backward that asks gets ONE torch.zeros over all reservations and every Function its slice of it."""

    def __init__(self):
        self.total, self.buf, self.taken = 0, None, set()

    def reserve(self, numel):
        if self.buf is not None:          # a forward running after a backward of the same arena has started (checkpointing)
            return None
        off = self.total
        self.total += (int(numel) + 63) // 64 * 64      # 256-byte aligned slices
        return off

    def take(self, off, numel, device):
        if off is None or off in self.taken:            # second backward through the same graph: its own fresh zeros
            return torch.zeros(numel, dtype=torch.float32, device=device)
        if self.buf is None:
            self.buf = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.taken.add(off)
        return self.buf[off:off + numel]


_zero_arena = None


@_contextlib.contextmanager
def zero_arena():
    global _zero_arena
    outer, _zero_arena = _zero_arena, ZeroArena()
    try:
        yield _zero_arena
    finally:
        _zero_arena = outer


def _reserve_zeros(numel):
    """forward side: -> token for _take_zeros (None outside zero_arena())"""
    return (_zero_arena, _zero_arena.reserve(numel)) if _zero_arena is not None else None


def _take_zeros(token, numel, device):
    """backward side: a zeroed fp32 buffer of `numel` elements"""
    if token is None:
        return torch.zeros(numel, dtype=torch.float32, device=device)
    return token[0].take(token[1], numel, device)


class _GroupGather(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, feat, idx):
        f = _f32c(feat)
        n, c = f.shape
        m, ns = idx.shape
        out = torch.empty(m, ns, c, dtype=torch.float32, device=f.device)
        with torch.cuda.device(f.device):
            _lib.call("fsg_group_gather_fwd_f32", _p(f), _p(idx), _p(out), n, c, m, ns, _stream())
        ctx.save_for_backward(idx)
        ctx.nc = (n, c)
        ctx.zeros = _reserve_zeros(n * c) if ctx.needs_input_grad[0] else None
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        n, c = ctx.nc
        m, ns = idx.shape
        g = _f32c(g)
        gf = _take_zeros(ctx.zeros, n * c, g.device).view(n, c)
        with torch.cuda.device(g.device):
            _lib.call("fsg_group_gather_bwd_f32", _p(g), _p(idx), _p(gf), n, c, m, ns, _stream())
        return gf, None


def group_gather(feat, idx):
    """feat (n,c), idx (m,ns) int32 -> (m,ns,c) = feat[idx]."""
    _need_gpu(feat, idx)
    return _GroupGather.apply(feat, idx.to(torch.int32).contiguous())


class _GroupXyzFeat(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, xyz, new_xyz, feat, idx):
        xyz, new_xyz, f = _f32c(xyz), _f32c(new_xyz), _f32c(feat)
        n, c = f.shape
        m, ns = idx.shape
        out = torch.empty(m, ns, 3 + c, dtype=torch.float32, device=f.device)
        with torch.cuda.device(f.device):
            _lib.call("fsg_group_xyz_feat_fwd_f32", _p(xyz), _p(new_xyz), _p(f), _p(idx), _p(out), n, c, m, ns, _stream())
        ctx.save_for_backward(idx)
        ctx.nc = (n, c)
        ctx.zeros = _reserve_zeros(n * c) if ctx.needs_input_grad[2] else None
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        n, c = ctx.nc
        m, ns = idx.shape
        g = _f32c(g)
        gf = _take_zeros(ctx.zeros, n * c, g.device).view(n, c)
        with torch.cuda.device(g.device):
            _lib.call("fsg_group_xyz_feat_bwd_f32", _p(g), _p(idx), _p(gf), n, c, m, ns, _stream())
        return None, None, gf, None


def group_xyz_feat(xyz, new_xyz, feat, idx):
    """pointops.queryandgroup(use_xyz=True) behind the kNN query: (m, ns, 3 + c) = [xyz[idx] - new_xyz | feat[idx]], one launch
    each way; gradient for `feat` only (the caller checks that the coordinates need none)."""
    _need_gpu(xyz, new_xyz, feat, idx)
    return _GroupXyzFeat.apply(xyz, new_xyz, feat, idx.to(torch.int32).contiguous())


class _RowsMax(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x):
        x = _f32c(x)
        m, ns, c = x.shape
        out = torch.empty(m, c, dtype=torch.float32, device=x.device)
        arg = torch.empty(m, c, dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("fsg_rows_max_fwd_f32", _p(x), _p(out), _p(arg), m, ns, c, _stream())
        ctx.save_for_backward(arg)
        ctx.ns = ns
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        m, c = arg.shape
        g = _f32c(g)
        gx = torch.empty(m, ctx.ns, c, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.call("fsg_rows_max_bwd_f32", _p(g), _p(arg), _p(gx), m, ctx.ns, c, _stream())
        return gx


def rows_max(x):
    """x (m, ns, c) -> (m, c): max over the ns neighbour rows (nn.MaxPool1d(ns) of TransitionDown), one launch each way"""
    _need_gpu(x)
    return _RowsMax.apply(x)


class _Interp(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, feat, idx, d2):
        f = _f32c(feat)
        n, c = f.shape
        m, k = idx.shape
        out = torch.empty(m, c, dtype=torch.float32, device=f.device)
        with torch.cuda.device(f.device):
            _lib.call("fsg_interp_fwd_f32", _p(f), _p(idx), _p(d2), _p(out), n, c, m, k, _stream())
        ctx.save_for_backward(idx, d2)
        ctx.nc = (n, c)
        ctx.zeros = _reserve_zeros(n * c)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        idx, d2 = ctx.saved_tensors
        n, c = ctx.nc
        m, k = idx.shape
        g = _f32c(g)
        gf = _take_zeros(ctx.zeros, n * c, g.device).view(n, c)
        with torch.cuda.device(g.device):
            _lib.call("fsg_interp_bwd_f32", _p(g), _p(idx), _p(d2), _p(gf), n, c, m, k, _stream())
        return gf, None, None


def interpolate(feat, idx, dist2):
    """pointops.interpolation's arithmetic as one launch: feat (n, c), idx / dist2 (m, k <= 8) of the k nearest coarse points
    (squared distances, as fsg_knn_segment_f32 returns them) -> (m, c) inverse-distance weighted mean of feat[idx]."""
    _need_gpu(feat, idx, dist2)
    if idx.shape != dist2.shape or idx.shape[1] > 8:
        raise ValueError(f"interpolate: idx {tuple(idx.shape)} / dist2 {tuple(dist2.shape)}: equal shapes, k <= 8")
    return _Interp.apply(feat, idx.to(torch.int32).contiguous(), _f32c(dist2))


class _VecAttn(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, v, pos, w, idx):
        v, pos, w = _f32c(v), _f32c(pos), _f32c(w)
        n, c = v.shape
        ns, cw = w.shape[1], w.shape[2]
        out = torch.empty(n, c, dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            _lib.call("fsg_vec_attn_fwd_f32", _p(v), _p(pos), _p(w), _p(idx), _p(out), n, ns, c, cw, _stream())
        ctx.save_for_backward(v, pos, w, idx)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        v, pos, w, idx = ctx.saved_tensors
        n, c = v.shape
        ns, cw = w.shape[1], w.shape[2]
        g = _f32c(g)
        gv = torch.zeros_like(v)
        gpos = torch.empty_like(pos)
        gw = torch.empty_like(w)
        with torch.cuda.device(v.device):
            _lib.call("fsg_vec_attn_bwd_f32", _p(v), _p(pos), _p(w), _p(idx), _p(g), _p(gv), _p(gpos), _p(gw), n, ns, c,
                      cw, _stream())
        return gv, gpos, gw, None


def vec_attn(v, pos, w, idx):
    """out[i,ch] = sum_j (v[idx[i,j],ch] + pos[i,j,ch]) * w[i,j,ch % cw]  (seg_model.py:50-52)."""
    _need_gpu(v, pos, w, idx)
    if pos.shape != (v.shape[0], idx.shape[1], v.shape[1]) or w.shape[:2] != pos.shape[:2] or v.shape[1] % w.shape[2]:
        raise ValueError(f"vec_attn: inconsistent shapes v{tuple(v.shape)} pos{tuple(pos.shape)} w{tuple(w.shape)}")
    return _VecAttn.apply(v, pos, w, idx.to(torch.int32).contiguous())


# ------------------------------------------------------------------ [Wq ; Wk ; Wv] of every PointTransformerLayer, one launch
class _PackQKV(torch.autograd.Function):
    """inputs: (Wq, Wk, Wv, bq, bk, bv) per layer -> outputs: (W_qkv (3c, c), b_qkv (3c)) per layer, all views of ONE buffer that
    one torch.cat fills (ATen copies up to 128 pieces per launch).  The backward hands views of the incoming gradients on: no
    launch, and it does not read them -- which is what lets the products' weight gradients be reduced late (gemm_small defer)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, *ts):
        L = len(ts) // 6
        ctx.cs = [ts[6 * i].shape for i in range(L)]
        arena = torch.cat([t.reshape(-1) for t in ts])
        outs, off = [], 0
        for i in range(L):
            co, ci = ctx.cs[i]
            outs.append(arena[off:off + 3 * co * ci].view(3 * co, ci))
            off += 3 * co * ci
            outs.append(arena[off:off + 3 * co])
            off += 3 * co
        return tuple(outs)

    @staticmethod
    @_amp_bwd
    def backward(ctx, *gs):
        res = []
        for i, (co, ci) in enumerate(ctx.cs):
            gw, gb = gs[2 * i], gs[2 * i + 1]
            res += [None] * 3 if gw is None else [gw[0:co], gw[co:2 * co], gw[2 * co:3 * co]]
            res += [None] * 3 if gb is None else [gb[0:co], gb[co:2 * co], gb[2 * co:3 * co]]
        return tuple(res)


_qkv_packs = None      # {id(layer): (W_qkv, b_qkv)} inside qkv_pack()


@_contextlib.contextmanager
def qkv_pack(layers):
    """packs the q / k / v weights and biases of `layers` (modules with linear_q / linear_k / linear_v of equal output width) for
    the duration of one forward; PointTransformerLayer.forward picks its pair up through packed_qkv(layer)"""
    global _qkv_packs
    outer = _qkv_packs
    ok = [m for m in layers if m.linear_q.weight.is_cuda and m.linear_q.bias is not None and
          m.linear_q.weight.shape == m.linear_k.weight.shape == m.linear_v.weight.shape]
    ts = [t for m in ok for t in (m.linear_q.weight, m.linear_k.weight, m.linear_v.weight, m.linear_q.bias, m.linear_k.bias,
                                  m.linear_v.bias)]
    packs = {}
    if ts:
        outs = _PackQKV.apply(*ts)
        for i, m in enumerate(ok):
            w, b = outs[2 * i], outs[2 * i + 1]
            w._fsg_grad_unread = (m.linear_q.weight, m.linear_k.weight, m.linear_v.weight)
            b._fsg_grad_unread = (m.linear_q.bias, m.linear_k.bias, m.linear_v.bias)
            packs[id(m)] = (w, b)
    _qkv_packs = packs
    try:
        yield
    finally:
        _qkv_packs = outer


def packed_qkv(layer):
    return _qkv_packs.get(id(layer)) if _qkv_packs is not None else None


# ------------------------------------------------------------------ fused PointTransformerLayer body (seg_model.py:38-53)
_PT_PARAM_NAMES = ("lp1_w", "lp1_b", "bnp_g", "bnp_b", "lp2_w", "lp2_b", "bn1_g", "bn1_b", "lw1_w", "lw1_b", "bn2_g", "bn2_b",
                   "lw2_w", "lw2_b")


class _PTAttn(torch.autograd.Function):
    """out = fused(grouping, linear_p, linear_w, softmax, aggregate)(p, idx, qkv; 14 parameters).  Only the (n,ns,c/8)
    tensors u1 and softmax weights are kept for the backward; gradients: qkv and the 14 parameters."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, p, idx, qkv, bns, *params):
        n, c3 = qkv.shape
        c, ns = c3 // 3, idx.shape[1]
        cs = c // 8
        dev = qkv.device
        bnp, bn1, bn2 = bns
        training = bnp.training or bnp.running_mean is None
        moms = [0.0, 0.0, 0.0]
        if training:
            for i, bn in enumerate(bns):
                if bn.track_running_stats and bn.num_batches_tracked is not None:
                    moms[i] = float(bump_bn_counter(bn))
        prm = _lib.PTLayerParams()
        for name, t in zip(_PT_PARAM_NAMES, params):
            setattr(prm, name, t.data_ptr())
        for tag, bn in (("bnp", bnp), ("bn1", bn1), ("bn2", bn2)):
            track = training and bn.track_running_stats and bn.running_mean is not None
            setattr(prm, tag + "_rm", bn.running_mean.data_ptr() if track else None)
            setattr(prm, tag + "_rv", bn.running_var.data_ptr() if track else None)
        prm.eps_p, prm.eps_1, prm.eps_2 = bnp.eps, bn1.eps, bn2.eps
        prm.mom_p, prm.mom_1, prm.mom_2 = moms
        if training:
            stats = torch.empty(2 * (3 + c + cs), dtype=torch.float32, device=dev)
        else:
            stats = torch.cat([t for bn in bns for t in (bn.running_mean.float(), torch.rsqrt(bn.running_var.float() + bn.eps))])
        out = torch.empty(n, c, dtype=torch.float32, device=dev)
        u1 = torch.empty(n, ns, cs, dtype=torch.float32, device=dev)
        sm = torch.empty(n, ns, cs, dtype=torch.float32, device=dev)
        ws = _lib.workspace("fsg_pt_attn", n, ns, c, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_pt_attn_fwd_f32", _p(p), _p(idx), _p(qkv), ctypes.c_void_p(qkv.data_ptr() + 4 * c),
                      ctypes.c_void_p(qkv.data_ptr() + 8 * c), c3, ctypes.byref(prm), n, ns, c, int(training), _p(out),
                      _p(stats), _p(u1), _p(sm), _p(ws), _stream())
        ctx.save_for_backward(p, idx, qkv, stats, u1, sm, *params)
        ctx.meta = (n, ns, c, training, (bnp.eps, bn1.eps, bn2.eps))
        ctx.zeros = _reserve_zeros(n * 3 * c + (n * 3 if ctx.needs_input_grad[0] else 0))
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        p, idx, qkv, stats, u1, sm, *params = ctx.saved_tensors
        n, ns, c, training, eps = ctx.meta
        dev = qkv.device
        prm = _lib.PTLayerParams()
        for name, t in zip(_PT_PARAM_NAMES, params):
            setattr(prm, name, t.data_ptr())
        prm.eps_p, prm.eps_1, prm.eps_2 = eps
        sizes = [t.numel() for t in params]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        grads, gstruct, off = [], _lib.PTLayerGrads(), 0
        for name, t, sz in zip(_PT_PARAM_NAMES, params, sizes):
            gt = flat[off:off + sz].view(t.shape)
            setattr(gstruct, name, gt.data_ptr())
            grads.append(gt)
            off += sz
        # dk / dv / dp are accumulated with atomics: ONE zero fill for both buffers (two fill launches per layer and step before)
        need_dp = ctx.needs_input_grad[0]
        zbuf = _take_zeros(ctx.zeros, n * 3 * c + (n * 3 if need_dp else 0), dev)
        dqkv = zbuf[:n * 3 * c].view(n, 3 * c)
        dp = zbuf[n * 3 * c:].view(n, 3) if need_dp else None
        ws = _lib.workspace("fsg_pt_attn", n, ns, c, device=dev)
        g = _f32c(g)
        with torch.cuda.device(dev):
            _lib.call("fsg_pt_attn_bwd_f32", _p(p), _p(idx), _p(qkv), ctypes.c_void_p(qkv.data_ptr() + 4 * c),
                      ctypes.c_void_p(qkv.data_ptr() + 8 * c), 3 * c, ctypes.byref(prm), n, ns, c, int(training), _p(g),
                      _p(stats), _p(u1), _p(sm), _p(dqkv), ctypes.c_void_p(dqkv.data_ptr() + 4 * c),
                      ctypes.c_void_p(dqkv.data_ptr() + 8 * c), 3 * c, _p(dp), ctypes.byref(gstruct), _p(ws), _stream())
        return (dp, None, dqkv, None, *grads)


PT_ATTN_PLANES = (32, 64, 128, 256, 512)


def pt_attn(p, idx, qkv, linear_p, linear_w):
    """Fused body of PointTransformerLayer.  p (n,3), idx (n,ns) int32, qkv (n,3c) = [q | k | v] rows;
    linear_p = Sequential(Linear(3,3), BatchNorm1d(3), ReLU, Linear(3,c)), linear_w = Sequential(BatchNorm1d(c), ReLU,
    Linear(c,c/8), BatchNorm1d(c/8), ReLU, Linear(c/8,c/8)) -- the reference's module layout (seg_model.py:27-33)."""
    _need_gpu(p, idx, qkv)
    c = qkv.shape[1] // 3
    if c not in PT_ATTN_PLANES or not 1 <= idx.shape[1] <= 16:
        raise ValueError(f"fused PointTransformer layer supports planes {PT_ATTN_PLANES} and nsample <= 16, got {c}, {idx.shape[1]}")
    lp1, bnp, _, lp2 = linear_p
    bn1, _, lw1, bn2, _, lw2 = linear_w
    params = (lp1.weight, lp1.bias, bnp.weight, bnp.bias, lp2.weight, lp2.bias, bn1.weight, bn1.bias, lw1.weight, lw1.bias,
              bn2.weight, bn2.bias, lw2.weight, lw2.bias)
    params = tuple(t if t.is_contiguous() else t.contiguous() for t in params)
    p = p if p.dtype == torch.float32 and p.is_contiguous() else p.float().contiguous()
    return _PTAttn.apply(p, idx.to(torch.int32).contiguous(), qkv.contiguous(), (bnp, bn1, bn2), *params)


# ------------------------------------------------------------------ image front end: Foerstner keypoints, MIND (csrc/volume.hip)
def gaussian_taps(sigma):
    """the taps of utils/image_utils.py:25-29 (N = 2 ceil(1.5 sigma) + 1, normalised in fp32), computed the same way, on the
    host -> (N,) fp32 CPU tensor"""
    s = torch.tensor([float(sigma)])
    n = int(torch.ceil(s * 3.0 / 2.0).long().item()) * 2 + 1
    w = torch.exp(-torch.pow(torch.linspace(-(n // 2), n // 2, n), 2) / (2 * torch.pow(s, 2)))
    w /= w.sum()
    return w


def _host_floats(t):
    vals = [float(v) for v in t.tolist()]
    return (ctypes.c_float * len(vals))(*vals), len(vals)


def _host_ints(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int * len(vals))(*vals)


def _volume(img, what="img"):
    """(B, 1, D, H, W) -> contiguous fp32 and its four sizes"""
    if img.dim() != 5 or img.shape[1] != 1:
        raise ValueError(f"expected {what} (B, 1, D, H, W), got {tuple(img.shape)}")
    v = _f32c(img)
    return v, (v.shape[0], v.shape[2], v.shape[3], v.shape[4])


def foerstner_distinctiveness(img, sigma):
    """data_processing/foerstner.py:62-73 in one launch (fsg_foerstner_dist_f32): img (B, 1, D, H, W) -> (B, 1, D, H, W).
    NaN where the smoothed structure tensor is singular, like the reference."""
    _need_gpu(img)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        w, n = _host_floats(gaussian_taps(sigma))
        out = torch.empty_like(v)
        with torch.cuda.device(v.device):
            _lib.call("fsg_foerstner_dist_f32", _p(v), B, D, H, W, w, n, _p(out), _stream())
    return out


def _mask_bytes(mask, shape):
    if mask is None:
        return None
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the volume {tuple(shape)}")
    return (mask != 0).to(torch.uint8).contiguous()


def nms_max(data, kernel_size):
    """utils/image_utils.py:38-50 (fsg_nms_keypoints): window maximum with the reference's asymmetric padding for even
    kernels; NaN propagates.  data (B, 1, D, H, W) -> same shape"""
    _need_gpu(data)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(data, "data")
        out = torch.empty_like(v)
        with torch.cuda.device(v.device):
            _lib.call("fsg_nms_keypoints", _p(v), None, B, D, H, W, int(kernel_size), 0.0, _p(out), None, _stream())
    return out


def nms_keypoint_flags(dist, mask, d, thresh):
    """foerstner.py:90-107 without the nonzero: eroded(mask) & (window max == dist) & (dist >= thresh) -> (B, 1, D, H, W) bool"""
    _need_gpu(dist, mask)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(dist, "dist")
        m = _mask_bytes(mask, v.shape)
        flags = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
        with torch.cuda.device(v.device):
            _lib.call("fsg_nms_keypoints", _p(v), _p(m), B, D, H, W, int(d), float(thresh), None, _p(flags), _stream())
    return flags.bool()


def _mind_tables(shifts, outch):
    nch = len(shifts)
    flat = [int(v) for pair in shifts for voxel in pair for v in (voxel if isinstance(voxel, (tuple, list)) else (voxel,))]
    return nch, _host_ints(flat), _host_ints(outch if outch is not None else range(nch))


def mind_mean(img, dilation, sigma, shifts, box):
    """statistics pass (fsg_mind_stats_f32): the mean over the batch volume of mean_c(ssd_c - min_c ssd_c) -> (1,) fp32 on the
    device.  `shifts`: per channel the two voxel offsets ((dz, dy, dx), (dz, dy, dx)) in {-1, 0, 1}; with `box`, per channel two
    27-bit subsets of the 3 x 3 x 3 stencil whose sums are compared."""
    _need_gpu(img)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        nch, sh, _ = _mind_tables(shifts, None)
        w, n = _host_floats(gaussian_taps(sigma))
        ws = _lib.workspace("fsg_mind_stats", B, D, H, W, device=v.device)
        mean = torch.empty(1, dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            _lib.call("fsg_mind_stats_f32", _p(v), B, D, H, W, int(dilation), nch, int(box), sh, w, n, _p(ws), _p(mean), _stream())
    return mean


def mind_volume(img, dilation, sigma, shifts, outch, box, mean=None):
    """statistics + evaluation pass for the whole volume -> (B, nch, D, H, W)"""
    _need_gpu(img)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        if mean is None:
            mean = mind_mean(v, dilation, sigma, shifts, box)
        nch, sh, oc = _mind_tables(shifts, outch)
        w, n = _host_floats(gaussian_taps(sigma))
        out = torch.empty(B, nch, D, H, W, dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            _lib.call("fsg_mind_eval_f32", _p(v), B, D, H, W, int(dilation), nch, int(box), sh, oc, w, n, _p(mean), _p(out),
                      _stream())
    return out


def mind_keypoints(img, kp, dilation, sigma, shifts, outch, box, mean=None):
    """statistics pass + evaluation at kp (K, 3) voxel indices (z, y, x) of ONE volume -> (nch, K); the feature volume is
    never written"""
    _need_gpu(img, kp)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        if B != 1:
            raise ValueError("mind_keypoints: one volume at a time")
        if kp.dim() != 2 or kp.shape[1] != 3 or kp.is_floating_point():
            raise ValueError(f"expected kp (K, 3) integer voxel indices, got {tuple(kp.shape)} {kp.dtype}")
        nch, sh, oc = _mind_tables(shifts, outch)
        K = kp.shape[0]
        out = torch.empty(nch, K, dtype=torch.float32, device=v.device)
        if K == 0:
            return out
        kpc = kp.detach().to(torch.int64).contiguous()
        lo, hi = kpc.amin(0).tolist(), kpc.amax(0).tolist()
        if min(lo) < 0 or any(h >= s for h, s in zip(hi, (D, H, W))):
            raise ValueError(f"keypoints span {lo}..{hi}, outside the volume {(D, H, W)}")
        if mean is None:
            mean = mind_mean(v, dilation, sigma, shifts, box)
        w, n = _host_floats(gaussian_taps(sigma))
        with torch.cuda.device(v.device):
            _lib.call("fsg_mind_eval_kp_f32", _p(v), D, H, W, int(dilation), nch, int(box), sh, oc, w, n, _p(mean), _p(kpc), K,
                      _p(out), _stream())
    return out


# ------------------------------------------------------------------ Hessian fissure enhancement (csrc/fissure_enhance.hip)
MAX_TAP_RADIUS = _lib.ENHANCE_MAX_TAP_RADIUS   # of the derivative taps (derivation sigma <= 1) and of the keypoint smoothing taps


def gaussian_derivative_taps(sigma, order, truncate=4.0):
    """utils/image_utils.py:53-58 (scipy's Gaussian kernel of derivative `order`, radius int(truncate sigma + 0.5)), computed
    the same way in fp64 on the host and cast -> (2 radius + 1,) fp32 CPU tensor"""
    import numpy as np
    sigma, order = float(sigma), int(order)
    if not sigma > 0 or order < 0:
        raise ValueError(f"gaussian_derivative_taps: sigma {sigma} must be positive and order {order} non-negative")
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    if order > 0:   # q <- q' + q p', p' = -x / sigma^2, applied to the coefficients of q `order` times
        exponents = np.arange(order + 1)
        q = np.zeros(order + 1)
        q[0] = 1
        step = np.diag(exponents[1:], 1) + np.diag(np.ones(order) / -(sigma * sigma), -1)
        for _ in range(order):
            q = step.dot(q)
        phi = (x[:, None] ** exponents).dot(q) * phi
    return torch.from_numpy(phi).float()


def discrete_gaussian_taps(variance, max_error=0.01, max_width=32, spacing=None):
    """the operator of ITK's DiscreteGaussianImageFilter as ITK documents it (GaussianOperator): coefficients exp(-t) I_k(t),
    t the variance in voxels, terms added until their sum reaches 1 - max_error (or the width reaches max_width), then
    normalised.  `variance` is a number or one per axis (z, y, x); with `spacing` (z, y, x) it is physical and becomes
    variance / spacing^2 per axis (useImageSpacing).  -> three fp32 CPU tensors (z, y, x).  Parity with SimpleITK itself is
    not pinned by a test; pass explicit taps to `smooth_threshold` to use SimpleITK's."""
    from scipy.special import ive
    var = [float(variance)] * 3 if not hasattr(variance, "__len__") else [float(v) for v in variance]
    sp = [1.0] * 3 if spacing is None else [float(s) for s in spacing]
    if len(var) != 3 or len(sp) != 3 or min(var) < 0 or min(sp) <= 0:
        raise ValueError(f"discrete_gaussian_taps: variance {variance} / spacing {spacing} must be three non-negative / positive numbers")
    taps = []
    for v, s in zip(var, sp):
        t = v / (s * s)
        half = [float(ive(0, t))]
        total = half[0]
        while total < 1.0 - max_error and 2 * len(half) + 1 <= max_width:
            half.append(float(ive(len(half), t)))
            total += 2 * half[-1]
        full = half[:0:-1] + half
        taps.append((torch.tensor(full, dtype=torch.float64) / total).float())
    return tuple(taps)


def _odd_taps(t, what):
    t = torch.as_tensor(t, dtype=torch.float32).detach().cpu().flatten()
    if t.numel() % 2 == 0 or t.numel() > 2 * MAX_TAP_RADIUS + 1:
        raise ValueError(f"{what}: {t.numel()} taps; the kernel takes an odd number, at most {2 * MAX_TAP_RADIUS + 1} "
                         f"(radius {MAX_TAP_RADIUS})")
    return t


def fissure_enhance_check_sigma(derivation_sigma):
    """the derivative taps of `derivation_sigma` must fit the kernel's radius (1..4): -> (k1, k2) fp32 CPU tensors"""
    k1, k2 = gaussian_derivative_taps(derivation_sigma, 1), gaussian_derivative_taps(derivation_sigma, 2)
    if k1.numel() > 2 * MAX_TAP_RADIUS + 1 or k1.numel() < 3:
        raise ValueError(f"fissure_enhance: derivation sigma {derivation_sigma} gives a tap radius of {k1.numel() // 2}; the "
                         f"kernel takes 1..{MAX_TAP_RADIUS} (sigma <= 1)")
    return k1, k2


def fissure_enhance(img, fissure_mu, fissure_sigma, derivation_sigma=1.0, mask=None, return_intermediate=False):
    """HessianEnhancementFilter.forward + fissure_filter (data_processing/fissure_enhancement.py:47-99, 149-180) in one launch
    (fsg_fissure_enhance_f32): img (B, 1, D, H, W) -> F of the same shape, times (mask != 0) when a mask of that shape is
    given; with `return_intermediate` -> (F, planeness, HU weight).  The derivation sigma is at most 1 (tap radius 4)."""
    k1, k2 = fissure_enhance_check_sigma(derivation_sigma)
    if not float(fissure_sigma) > 0:
        raise ValueError(f"fissure_enhance: fissure_sigma {fissure_sigma} must be positive")
    _need_gpu(img, mask)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(img)
        if mask is not None and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous() and mask.shape == v.shape:
            m = mask.view(torch.uint8)          # the kernel tests the byte against 0: no dense conversion pass
        else:
            m = _mask_bytes(mask, v.shape)
        out = torch.empty_like(v)
        P, hw = (torch.empty_like(v), torch.empty_like(v)) if return_intermediate else (None, None)
        w1, n = _host_floats(k1)
        w2, _ = _host_floats(k2)
        with torch.cuda.device(v.device):
            _lib.call("fsg_fissure_enhance_f32", _p(v), _p(m), B, D, H, W, w1, w2, n, float(fissure_mu), float(fissure_sigma),
                      _p(out), _p(P), _p(hw), _stream())
    return (out, P, hw) if return_intermediate else out


def smooth_threshold(vol, taps, thresh, return_flags=True):
    """fsg_smooth_threshold_f32: vol (B, 1, D, H, W) smoothed separably with `taps` = (taps_z, taps_y, taps_x) (odd counts,
    radius <= 4; axis order 0, 1, 2; replicate padding) -> (values, flags): the smoothed value where it exceeds `thresh` and 0
    elsewhere, and that comparison as (B, 1, D, H, W) bool (values alone with return_flags=False)"""
    if len(taps) != 3:
        raise ValueError("smooth_threshold: expected three tap vectors (z, y, x)")
    host = [_host_floats(_odd_taps(t, f"smooth_threshold: axis {ax}")) for ax, t in enumerate(taps)]
    _need_gpu(vol)
    with torch.no_grad():
        v, (B, D, H, W) = _volume(vol, "vol")
        out = torch.empty_like(v)
        flags = torch.empty(v.shape, dtype=torch.uint8, device=v.device) if return_flags else None
        with torch.cuda.device(v.device):
            _lib.call("fsg_smooth_threshold_f32", _p(v), B, D, H, W, host[0][0], host[0][1], host[1][0], host[1][1], host[2][0],
                      host[2][1], float(thresh), _p(out), _p(flags), _stream())
    return (out, flags.view(torch.bool)) if return_flags else out   # the kernel writes 0 or 1: a view, not a pass


# ------------------------------------------------------------------ random-walker filling, lobes to fissures (csrc/random_walk.hip)
def _rw_volumes(im, labels, mask, edge_weights):
    """checks and packs the three volumes of a random-walker solve: (B, D, H, W) or one (D, H, W) / (H, W) image ->
    (im bytes or fp32, labels uint8 or int32, mask bytes or None, mode, (B, D, H, W), the caller's volume shape)"""
    if edge_weights not in ("binary", "intensity"):
        raise ValueError(f'No edge weights named "{edge_weights}" known.')
    if im.dim() not in (2, 3, 4):
        raise ValueError(f"expected im (H, W), (D, H, W) or (B, D, H, W), got {tuple(im.shape)}")
    if labels.shape != im.shape or (mask is not None and mask.shape != im.shape):
        raise ValueError(f"im {tuple(im.shape)}, labels {tuple(labels.shape)} and mask "
                         f"{None if mask is None else tuple(mask.shape)} must have one shape")
    if labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor (0 = no seed), got {labels.dtype}")
    _need_gpu(im, labels, mask)
    shape = tuple(im.shape)
    full = (1,) * (4 - im.dim()) + shape if im.dim() < 4 else shape
    if edge_weights == "binary":
        if im.dtype in (torch.bool, torch.uint8):
            imc = im.contiguous().view(torch.uint8)
        else:   # the kernel compares bytes: number the distinct values (one sort; lobe and fissure images have a handful)
            values, inverse = torch.unique(im, return_inverse=True)
            if values.numel() > 256:
                raise ValueError(f"'binary' edge weights compare bytes: im has {values.numel()} distinct values, at most 256 are "
                                 f"supported")
            imc = inverse.to(torch.uint8).contiguous()
        mode = _lib.RW_BINARY
    else:
        imc, mode = _f32c(im), _lib.RW_INTENSITY
    lc = labels.detach().contiguous() if labels.dtype in (torch.uint8, torch.int32) else labels.detach().to(torch.int32).contiguous()
    mc = None if mask is None else (mask.contiguous().view(torch.uint8) if mask.dtype in (torch.bool, torch.uint8)
                                    else (mask != 0).view(torch.uint8))
    return imc.view(full), lc.view(full), None if mc is None else mc.view(full), mode, full, shape


def _rw_solve(im, labels, mask, edge_weights, tol, max_iter, check_every, num_labels, want_prob, want_filled):
    import warnings
    if not (tol >= 0 and max_iter >= 0 and check_every >= 1):
        raise ValueError(f"random_walk_solve: tol {tol} / max_iter {max_iter} / check_every {check_every}")
    with torch.no_grad():
        imc, lc, mc, mode, (B, D, H, W), shape = _rw_volumes(im, labels, mask, edge_weights)
        dev = imc.device
        if num_labels is None:   # random_walk.py:108: the largest seeded label (one reduction, one host read)
            seeded = lc if mc is None else torch.where(mc != 0, lc, torch.zeros_like(lc))
            if int(seeded.min()) < 0:
                raise ValueError("random_walk_solve: negative labels")
            num_labels = int(seeded.max())
        K = int(num_labels)
        if not 1 <= K <= _lib.RW_MAX_LABELS:
            raise ValueError(f"random_walk_solve: {K} labels; the kernels are built for 1..{_lib.RW_MAX_LABELS} (and need a seed)")
        ws = _lib.workspace("fsg_random_walk", B, K, D, H, W, device=dev)
        nbytes = ws.numel()
        stop = torch.empty(B * K, dtype=torch.int32, device=dev)
        relres = torch.empty(B * K, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_random_walk_prep", _p(imc), mode, _p(lc), int(lc.dtype == torch.int32), _p(mc), B, K, D, H, W, _p(ws),
                      nbytes, _p(stop), _p(relres), _stream())
            done = 0
            while done < max_iter:   # the host looks at the stopping iterates once per `check_every` iterations
                n = min(int(check_every), max_iter - done)
                _lib.call("fsg_random_walk_iterate", _p(imc), mode, B, K, D, H, W, done, n, float(tol), _p(ws), nbytes, _p(stop),
                          _p(relres), _stream())
                done += n
                if bool((stop >= 0).all()):
                    break
            prob = torch.empty(B, D, H, W, K, dtype=torch.float32, device=dev) if want_prob else None
            filled = torch.empty(B, D, H, W, dtype=torch.uint8, device=dev) if want_filled else None
            _lib.call("fsg_random_walk_finish", B, K, D, H, W, _p(ws), nbytes, _p(prob), _p(filled), _stream())
        iters = torch.where(stop >= 0, stop, torch.full_like(stop, done)).view(B, K)
        if bool((stop < 0).any()):
            warnings.warn(f"random_walk_solve: {int((stop < 0).sum())} of {B * K} systems did not reach tol = {tol} in max_iter = "
                          f"{max_iter} iterations (largest relative residual {float(relres.max()):.3g})", RuntimeWarning)
    lead = shape[:-3] if len(shape) == 4 else ()
    info = dict(iterations=iters.view(*lead, K), relative_residual=relres.view(*lead, K), num_labels=K)
    return (None if prob is None else prob.view(*shape, K)), (None if filled is None else filled.view(shape)), info


def random_walk_solve(im, labels, mask, edge_weights, tol=1e-3, max_iter=5000, check_every=25, num_labels=None, return_info=False):
    """compute_laplace_matrix + random_walk (data_processing/random_walk.py:15-116) without the matrix: the probabilities of
    the random walker seeded by `labels` (integers, 0 = no seed) inside `mask` (None: everywhere) on the image graph of `im`
    with 'binary' or 'intensity' edge weights.  im / labels / mask (D, H, W), (H, W) or a batch (B, D, H, W) -> (..., K) fp32:
    one-hot rows at seeds, the solution at the other voxels of the mask, 0 outside.  K = `num_labels` or the largest seeded
    label (one host read).  Jacobi-preconditioned conjugate gradients on all B K systems at once; a system stops at
    |r| <= tol |b| and is then left alone, so a batch item's result equals its own run bit for bit.  The host looks every
    `check_every` iterations; reaching `max_iter` warns.  With `return_info` -> (prob, dict(iterations (..., K): the iterate
    at which each system stopped -- the true one, not rounded up to `check_every` --, relative_residual (..., K), num_labels))."""
    prob, _, info = _rw_solve(im, labels, mask, edge_weights, tol, max_iter, check_every, num_labels, True, False)
    return (prob, info) if return_info else prob


def random_walk_fill(labels, mask, tol=1e-3, max_iter=5000, check_every=25, num_labels=None, return_info=False):
    """fill_lobes (data_processing/find_lobes.py:17-30): the 'binary' graph of (labels != 0), the walker seeded by `labels`,
    first-index argmax + 1 inside the mask and 0 outside -> uint8 of the shape of `labels`; the probabilities are not written"""
    _, filled, info = _rw_solve(labels != 0, labels, mask, "binary", tol, max_iter, check_every, num_labels, False, True)
    return (filled, info) if return_info else filled


def lobes_to_fissures_labels(lobes_filled):
    """the tensor part of lobes_to_fissures (find_lobes.py:47-88) in one launch on labels (fsg_lobes_to_fissures_u8): a lobe
    is present at a voxel if the voxel or one of its six neighbours carries it; fissure 1 between lobes 3 and 4, 2 between 1 and
    2 (and 1 and 5), 3 between 2 and 5, later ones overwriting.  lobes_filled (D, H, W) or (B, D, H, W) integers -> uint8.
    The number of lobes is the largest label (one host read); fewer than 4 is a ValueError."""
    if lobes_filled.dim() not in (3, 4) or lobes_filled.is_floating_point() or lobes_filled.dtype == torch.bool:
        raise ValueError(f"expected integer labels (D, H, W) or (B, D, H, W), got {tuple(lobes_filled.shape)} {lobes_filled.dtype}")
    _need_gpu(lobes_filled)
    with torch.no_grad():
        lo, hi = int(lobes_filled.min()), int(lobes_filled.max())
        if lo < 0 or hi > 31:
            raise ValueError(f"lobes_to_fissures_labels: labels span {lo}..{hi}, outside 0..31")
        if hi < 4:
            raise ValueError(f"lobes_to_fissures_labels: the largest label is {hi}; the fissures are defined for 4 or 5 lobes")
        lc = lobes_filled.detach().to(torch.uint8).contiguous()
        D, H, W = lc.shape[-3:]
        B = lc.shape[0] if lc.dim() == 4 else 1
        out = torch.empty_like(lc)
        with torch.cuda.device(lc.device):
            _lib.call("fsg_lobes_to_fissures_u8", _p(lc), B, D, H, W, hi, _p(out), _stream())
    return out


# ------------------------------------------------------------------ ball morphology, connected components (csrc/morphology.hip)
def _radius3(radius):
    """an int or three ints (rz, ry, rx), each 0..8"""
    if isinstance(radius, int) and not isinstance(radius, bool):
        r = (radius,) * 3
    else:
        r = tuple(radius) if isinstance(radius, (tuple, list)) else ()
    if len(r) != 3 or any(not isinstance(x, int) or isinstance(x, bool) for x in r):
        raise ValueError(f"radius must be an int or three ints (rz, ry, rx), got {radius!r}")
    if any(x < 0 or x > _lib.MORPH_MAX_RADIUS for x in r):
        raise ValueError(f"radius {r} outside 0..{_lib.MORPH_MAX_RADIUS}")
    return r


def ball_offsets(radius):
    """the offsets (n, 3) int64 (dz, dy, dx), in raster order, of the ball structuring element of per-axis radius
    (rz, ry, rx): sum_i (o_i / (r_i + 0.5))^2 <= 1 (an axis of radius 0 contributes only 0) -- the definition used here in
    place of sitk.sitkBall (parity with SimpleITK is unpinned).  Decided in integers: with m = 2 r + 1 the
    test is 4 sum_i o_i^2 prod_{j != i} m_j^2 <= prod_j m_j^2, whose sides have different parity."""
    rz, ry, rx = _radius3(radius)
    mz, my, mx = (2 * rz + 1) ** 2, (2 * ry + 1) ** 2, (2 * rx + 1) ** 2
    offs = [(dz, dy, dx) for dz in range(-rz, rz + 1) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)
            if 4 * (dz * dz * my * mx + dy * dy * mz * mx + dx * dx * mz * my) <= mz * my * mx]
    return torch.tensor(offs, dtype=torch.int64)


def _binary_volume(vol, what):
    """(D, H, W) or (B, D, H, W), bool or integer -> the tensor as (B, D, H, W) and whether it came without a batch axis"""
    if vol.dim() not in (3, 4) or vol.is_floating_point() or vol.is_complex():
        raise ValueError(f"{what}: expected a bool or integer volume (D, H, W) or (B, D, H, W), got {tuple(vol.shape)} {vol.dtype}")
    if vol.numel() == 0:
        raise ValueError(f"{what}: empty volume {tuple(vol.shape)}")
    _need_gpu(vol)
    return (vol[None] if vol.dim() == 3 else vol), vol.dim() == 3


def _pack_bits(v4, value=None):
    """(B, D, H, W) bool / integer on the device -> bit plane (B, D, H, ceil(W / 64)) int64: voxel != 0, or == value (0..255
    on a uint8 volume)"""
    if v4.dtype == torch.bool:
        src = v4.contiguous().view(torch.uint8)
    elif v4.dtype == torch.uint8:
        src = v4.contiguous()
    elif value is None:
        src = (v4 != 0).contiguous().view(torch.uint8)       # (a comparison keeps the strides of a permuted input)
    else:
        src, value = (v4 == value).contiguous().view(torch.uint8), None
    B, D, H, W = src.shape
    bits = torch.empty(B, D, H, (W + 63) // 64, dtype=torch.int64, device=src.device)
    with torch.cuda.device(src.device):
        _lib.call("fsg_bits_pack_u8", _p(src), B, D, H, W, -1 if value is None else int(value), _p(bits), _stream())
    return bits


def _unpack_bits(bits, W):
    B, D, H, _ = bits.shape
    out = torch.empty(B, D, H, W, dtype=torch.uint8, device=bits.device)
    with torch.cuda.device(bits.device):
        _lib.call("fsg_bits_unpack_u8", _p(bits), B, D, H, W, _p(out), _stream())
    return out.view(torch.bool)   # the kernel writes 0 or 1: a view, not a pass


def _bits_dilate(bits, W, r, border=0, inv_in=False, inv_out=False):
    """one launch on a bit plane: [not] dilate([not] bits) with the ball of radius r = (rz, ry, rx) and the border value"""
    B, D, H, _ = bits.shape
    out = torch.empty_like(bits)
    with torch.cuda.device(bits.device):
        _lib.call("fsg_ball_dilate_bits", _p(bits), B, D, H, W, r[0], r[1], r[2], int(border), int(inv_in), int(inv_out), _p(out),
                  _stream())
    return out


def _bits_erode(bits, W, r, border=1):
    """erosion = the complement of the dilation of the complement with the complementary border (the ball is symmetric)"""
    return _bits_dilate(bits, W, r, border=1 - int(border), inv_in=True, inv_out=True)


def _bits_window(bits, W, offset, out_dhw):
    """the box of size out_dhw whose corner sits at `offset` of the volume (negative: padding with 0), in bit-plane space"""
    B, D, H, _ = bits.shape
    Do, Ho, Wo = out_dhw
    out = torch.empty(B, Do, Ho, (Wo + 63) // 64, dtype=torch.int64, device=bits.device)
    with torch.cuda.device(bits.device):
        _lib.call("fsg_bits_window", _p(bits), B, D, H, W, offset[0], offset[1], offset[2], Do, Ho, Wo, _p(out), _stream())
    return out


def _bits_closing(bits, W, r):
    """closing on the zero-extended infinite grid, cropped: the dilation is also formed r voxels outside the volume (the
    plane is padded in bit space, never as bytes), so the erosion sees what it would on the infinite grid"""
    B, D, H, _ = bits.shape
    Wp = W + 2 * r[2]
    padded = _bits_window(bits, W, (-r[0], -r[1], -r[2]), (D + 2 * r[0], H + 2 * r[1], Wp))
    closed = _bits_erode(_bits_dilate(padded, Wp, r, border=0), Wp, r, border=0)
    return _bits_window(closed, Wp, r, (D, H, W))


def _bits_opening(bits, W, r):
    """dilate(erode(x, border 0), border 0): what the zero-extended infinite grid gives, cropped"""
    return _bits_dilate(_bits_erode(bits, W, r, border=0), W, r, border=0)


def _morph_public(vol, radius, what, op):
    r = _radius3(radius)
    v4, squeeze = _binary_volume(vol, what)
    with torch.no_grad():
        out = _unpack_bits(op(_pack_bits(v4), v4.shape[-1], r), v4.shape[-1])
    return out[0] if squeeze else out


def _border01(border):
    if border not in (0, 1, False, True):
        raise ValueError(f"border must be 0 or 1, got {border!r}")
    return int(border)


def binary_dilate(vol, radius, border=0):
    """sitk.BinaryDilate with a ball (find_lobes.py:123): vol (D, H, W) or (B, D, H, W), bool or integer (nonzero = set) ->
    bool.  radius an int or (rz, ry, rx), each 0..8, the ball of `ball_offsets`; `border` is the value outside the volume."""
    b = _border01(border)
    return _morph_public(vol, radius, "binary_dilate", lambda bits, W, r: _bits_dilate(bits, W, r, border=b))


def binary_erode(vol, radius, border=1):
    """sitk.BinaryErode with a ball (find_lobes.py:118; its boundary counts as foreground, hence border = 1)"""
    b = _border01(border)
    return _morph_public(vol, radius, "binary_erode", lambda bits, W, r: _bits_erode(bits, W, r, border=b))


def binary_closing(vol, radius):
    """sitk.BinaryMorphologicalClosing with a ball (find_lobes.py:122) on the zero-extended infinite grid, cropped"""
    return _morph_public(vol, radius, "binary_closing", _bits_closing)


def binary_opening(vol, radius):
    """sitk.BinaryMorphologicalOpening with a ball (find_lobes.py:128) on the zero-extended infinite grid, cropped"""
    return _morph_public(vol, radius, "binary_opening", _bits_opening)


def _thin_slice_fits(H, W):
    words = H * ((W + 63) // 64)
    if words > _lib.THIN_MAX_WORDS:
        raise ValueError(f"binary_thinning: a slice of {H} x {W} voxels is {words} words of 64 voxels, at most "
                         f"{_lib.THIN_MAX_WORDS} (H * ceil(W / 64)) fit in LDS")


def _bits_thin(bits, W, want_iterations=False):
    """one launch on a bit plane (csrc/thinning.hip): every slice thinned in its (y, x) plane until a pair of steps clears
    nothing -> (thinned plane, (B, D) int32 pair counts or None).  No host read."""
    B, D, H, _ = bits.shape
    _thin_slice_fits(H, W)
    out = torch.empty_like(bits)
    iters = torch.empty(B, D, dtype=torch.int32, device=bits.device) if want_iterations else None
    with torch.cuda.device(bits.device):
        _lib.call("fsg_thin_bits", _p(bits), B, D, H, W, _p(out), _p(iters), _stream())
    return out, iters


def binary_thinning(vol, return_iterations=False):
    """sitk.BinaryThinning as poisson_reconstruction uses it (data_processing/surface_fitting.py:109): vol (D, H, W) or
    (B, D, H, W), bool or integer (nonzero = set), any strides -> bool of the same shape; the input is not modified.  The
    two-sub-iteration thinning of Gonzalez & Woods in the (y, x) plane of every slice, clamped borders: slices never
    interact, so a sheet that crosses the slices becomes a one-voxel-wide sheet, not a curve.  The rule of csrc/thinning.hip
    and tests/thinning_oracle.py is the authority, parity with SimpleITK is unpinned.  A slice may hold at most
    `_lib.THIN_MAX_WORDS` words, H * ceil(W / 64) (ValueError beyond).  return_iterations: also the int32 (D) or (B, D)
    numbers of step pairs that cleared something, on the device.  One launch between the pack and the unpack, no host read."""
    v4, squeeze = _binary_volume(vol, "binary_thinning")
    W = v4.shape[-1]
    _thin_slice_fits(v4.shape[-2], W)        # before any work
    with torch.no_grad():
        bits, iters = _bits_thin(_pack_bits(v4), W, return_iterations)
        out = _unpack_bits(bits, W)
    if squeeze:
        out, iters = out[0], (iters[0] if return_iterations else None)
    return (out, iters) if return_iterations else out


def _cc_bits(bits, W, connectivity):
    """bit plane -> (labels (B, D, H, W) int32, n (B) int32 on the device): no host read"""
    B, D, H, _ = bits.shape
    dev = bits.device
    ws = _lib.workspace("fsg_cc", B, D, H, W, device=dev)
    labels = torch.empty(B, D, H, W, dtype=torch.int32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fsg_cc_label_bits", _p(bits), B, D, H, W, int(connectivity), _p(labels), _p(n), _p(ws), ws.numel(), _stream())
    return labels, n


def _stats_device(labels4, cap):
    """(B, D, H, W) int32 labels -> (B, cap, 4) int64 on the device: count, sum z, sum y, sum x of the labels 1..cap"""
    B, D, H, W = labels4.shape
    stats = torch.empty(B, cap, 4, dtype=torch.int64, device=labels4.device)
    with torch.cuda.device(labels4.device):
        _lib.call("fsg_component_stats_i32", _p(labels4), B, D, H, W, int(cap), _p(stats), _stream())
    return stats


def _labels_volume(labels, what):
    if labels.dim() not in (3, 4) or labels.dtype != torch.int32:
        raise ValueError(f"{what}: expected int32 labels (D, H, W) or (B, D, H, W), got {tuple(labels.shape)} {labels.dtype}")
    _need_gpu(labels)
    return (labels[None] if labels.dim() == 3 else labels).contiguous(), labels.dim() == 3


def _count(n, B, what):
    """n as given to component_stats / relabel_by_size: an int, or one int per item -> the capacity max(n, 1)"""
    ns = [n] if isinstance(n, int) else list(n)
    if any(not isinstance(x, int) or x < 0 for x in ns) or len(ns) not in (1, B):
        raise ValueError(f"{what}: n must be a non-negative int (or one per item), got {n!r}")
    return max(max(ns), 1)


def connected_components(mask, connectivity=6):
    """sitk.ConnectedComponentImageFilter (find_lobes.py:130-132; 6 is its default, fullyConnected is 26): mask (D, H, W) or
    (B, D, H, W), bool or integer (nonzero = object) -> (labels int32, n).  Components are numbered 1..n in raster order of
    their first voxel, as scipy.ndimage.label numbers them; n is an int, or a list of B ints for a batch (one host read)."""
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    v4, squeeze = _binary_volume(mask, "connected_components")
    with torch.no_grad():
        labels, n = _cc_bits(_pack_bits(v4), v4.shape[-1], connectivity)
        n = n.tolist()
    return (labels[0], n[0]) if squeeze else (labels, n)


def component_stats(labels, n):
    """sizes and index sums of the labels 1..n (RelabelComponentImageFilter's sizes, LabelShapeStatisticsImageFilter's
    centroids before the division; find_lobes.py:141-158): labels int32 (D, H, W) -> (sizes (n) int64, index_sums (n, 3)
    int64 in (z, y, x) order), on the device, exact; a batch (B, D, H, W) with n = max over the items -> (B, n), (B, n, 3).
    No host read."""
    l4, squeeze = _labels_volume(labels, "component_stats")
    cap = _count(n, l4.shape[0], "component_stats")
    n_max = max([n] if isinstance(n, int) else list(n))
    with torch.no_grad():
        stats = _stats_device(l4, cap)[:, :n_max]
    sizes, sums = stats[..., 0], stats[..., 1:]
    return (sizes[0], sums[0]) if squeeze else (sizes, sums)


def _size_order_lut(sizes):
    """(B, n) int64 sizes -> lut (B, n + 1) int32: old label -> rank by size, largest first, ties by the smaller label (a
    stable sort)"""
    B, n = sizes.shape
    order = torch.sort(sizes, dim=1, descending=True, stable=True).indices           # order[b, new - 1] = old - 1
    lut = torch.zeros(B, n + 1, dtype=torch.int32, device=sizes.device)
    lut.scatter_(1, order + 1, torch.arange(1, n + 1, dtype=torch.int32, device=sizes.device).expand(B, n).contiguous())
    return lut


def _apply_lut(l4, lut, out_dtype=torch.int32):
    B = l4.shape[0]
    out = torch.empty(l4.shape, dtype=out_dtype, device=l4.device)
    lut = lut.contiguous()
    with torch.cuda.device(l4.device):
        _lib.call("fsg_relabel_lut_i32", _p(l4), B, l4[0].numel(), _p(lut), lut.shape[1], _p(out), int(out_dtype == torch.int64),
                  _stream())
    return out


def relabel_by_size(labels, n):
    """sitk.RelabelComponentImageFilter with SortByObjectSize (find_lobes.py:141-143): label 1 becomes the largest component;
    equal sizes keep the order of their labels (this rule is ours, ITK's is unpinned).  labels int32 with values 0..n -> int32.
    Items of a batch whose count is below n have empty trailing labels, which sort last.  No host read."""
    l4, squeeze = _labels_volume(labels, "relabel_by_size")
    cap = _count(n, l4.shape[0], "relabel_by_size")
    with torch.no_grad():
        lut = _size_order_lut(_stats_device(l4, cap)[..., 0])
        out = _apply_lut(l4, lut)
    return out[0] if squeeze else out


# ------------------------------------------------------------------ Euclidean distance transform (csrc/edt.hip)
EDT_MAX_DIM = _lib.EDT_MAX_DIM
EDT_MAX_LABELS = _lib.EDT_MAX_LABELS
EDT_INT_INF = 2 ** 31 - 1    # the int32 mode's +inf


def _edt_shape(shape, what):
    D, H, W = (int(v) for v in shape[-3:])
    if max(D, H, W) > EDT_MAX_DIM or D * H * W >= 2 ** 31:
        raise ValueError(f"{what}: volume {(D, H, W)}: a dimension above {EDT_MAX_DIM} or 2^31 voxels or more")


def _edt_sampling(sampling, what):
    """None -> None (unit spacing: the int32 mode); a number or three (s0, s1, s2) for (D, H, W) -> three floats rounded to
    fp32, what the kernel computes with"""
    if sampling is None:
        return None
    s = (sampling,) * 3 if isinstance(sampling, (int, float)) and not isinstance(sampling, bool) else tuple(sampling)
    if len(s) != 3:
        raise ValueError(f"{what}: sampling must be None, a number or three numbers for (D, H, W), got {sampling!r}")
    s = tuple(float(torch.tensor(float(v), dtype=torch.float32)) for v in s)
    if any(not (0.0 < v <= 1e6) for v in s):
        raise ValueError(f"{what}: sampling {sampling!r} must be positive and at most 1e6")
    return s


def _edt_bits(bits, W, sampling, want_idx):
    """bit plane (B, D, H, WW) -> (d2 (B, D, H, W) int32 for unit spacing / fp32, site index (B, D, H, W) int32 or None).  Three
    launches on the current stream, no host read."""
    B, D, H, _ = bits.shape
    dev = bits.device
    d2 = torch.empty(B, D, H, W, dtype=torch.int32 if sampling is None else torch.float32, device=dev)
    idx = torch.empty(B, D, H, W, dtype=torch.int32, device=dev) if want_idx else None
    ws = _lib.workspace("fsg_edt", B, D, H, W, int(want_idx), device=dev)
    with torch.cuda.device(dev):
        if sampling is None:
            _lib.call("fsg_edt_sq_i32", _p(bits), B, D, H, W, _p(d2), _p(idx), _p(ws), ws.numel(), _stream())
        else:
            _lib.call("fsg_edt_sq_f32", _p(bits), B, D, H, W, sampling[0], sampling[1], sampling[2], _p(d2), _p(idx), _p(ws),
                      ws.numel(), _stream())
    return d2, idx


def distance_transform_edt(vol, sampling=None, return_distances=True, return_indices=False, squared=False):
    """scipy.ndimage.distance_transform_edt on the device (process_lung_mask.py:85): vol (D, H, W) or (B, D, H, W), bool or
    integer, nonzero = set; every voxel gets the Euclidean distance to the nearest zero voxel (a SITE) of its item, under
    `sampling` = None (unit), a number, or (s0, s1, s2) for (D, H, W).  Exact and separable (csrc/edt.hip).

    Distances are float32 square roots of the squared values; `squared=True` returns the squared values themselves: int32,
    exact, for sampling=None, else float32 (each term fl(fl(s * delta)^2), sums rounded once, no fused multiply-add; the
    spacings are rounded to fp32 first).  Indices are (3, D, H, W) int32 -- (B, 3, D, H, W) for a batch -- the (z, y, x) of the
    site that won.  Returns the distances, the indices, or (distances, indices), as scipy does.

    Where this is NOT scipy: an item without a zero voxel gives +inf distances (2^31 - 1 as squared int32) and -1 indices
    (scipy returns garbage there); among equidistant sites the winner is, per pass (W, then H, then D), the one with the
    smaller offset and then the lower index, which is not scipy's choice."""
    if not (return_distances or return_indices):
        raise ValueError("distance_transform_edt: at least one of return_distances / return_indices must be set")
    if vol.dim() in (3, 4):
        _edt_shape(vol.shape, "distance_transform_edt")
    s = _edt_sampling(sampling, "distance_transform_edt")
    v4, squeeze = _binary_volume(vol, "distance_transform_edt")
    B, D, H, W = v4.shape
    with torch.no_grad():
        d2, idx = _edt_bits(_pack_bits(v4), W, s, return_indices)
        out = []
        if return_distances:
            if squared:
                dist = d2
            else:
                dist = d2.to(torch.float32).sqrt_()
                if s is None:
                    dist.masked_fill_(d2 == EDT_INT_INF, float("inf"))
            out.append(dist[0] if squeeze else dist)
        if return_indices:
            x = idx % W
            y = torch.div(idx, W, rounding_mode="floor") % H
            z = torch.div(idx, H * W, rounding_mode="floor")
            zyx = torch.stack((z, y, x), 1)
            zyx.masked_fill_((idx < 0)[:, None], -1)
            out.append(zyx[0] if squeeze else zyx)
    return out[0] if len(out) == 1 else tuple(out)


def nearest_label(labels, candidates, sampling=None, keep=None):
    """For every voxel of `labels` (D, H, W), integer, the member of `candidates` whose nearest voxel is closest (Euclidean,
    under `sampling` as in `distance_transform_edt`) -> int32 (D, H, W).  On an exact tie the lowest label wins, as np.argmin
    over the distance maps in label order does (process_lung_mask.py:83-87; the feature transform has another tie rule and
    cannot stand in).  One batched distance transform over len(candidates) bit planes and one compare launch; with unit
    spacing the compare is exact in integers.  A candidate without voxels is infinitely far; if none has any, the lowest is
    returned.  `keep` (D, H, W), bool or uint8: voxels where it is 0 get 0 (process_lung_mask.py:88).  No host read."""
    cands = sorted({int(c) for c in candidates})
    if not cands or len(cands) > EDT_MAX_LABELS or len(cands) != len(list(candidates)):
        raise ValueError(f"nearest_label: candidates must be 1..{EDT_MAX_LABELS} distinct integers, got {candidates!r}")
    if labels.dim() != 3 or labels.is_floating_point() or labels.is_complex() or labels.numel() == 0:
        raise ValueError(f"nearest_label: expected an integer label map (D, H, W), got {tuple(labels.shape)} {labels.dtype}")
    _edt_shape(labels.shape, "nearest_label")
    s = _edt_sampling(sampling, "nearest_label")
    _need_gpu(labels, keep)
    if keep is not None and (keep.shape != labels.shape or keep.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"nearest_label: keep must be bool or uint8 of shape {tuple(labels.shape)}")
    D, H, W = labels.shape
    dev = labels.device
    with torch.no_grad():
        cand_t = torch.tensor(cands, dtype=torch.int32, device=dev)
        planes = labels[None] != cand_t[:, None, None, None]       # (K, D, H, W) bool; the comparison promotes, never wraps
        d2, _ = _edt_bits(_pack_bits(planes), W, s, False)          # a candidate's voxels are the sites of its plane
        out = torch.empty(D, H, W, dtype=torch.int32, device=dev)
        k8 = None if keep is None else keep.contiguous().view(torch.uint8)
        with torch.cuda.device(dev):
            _lib.call("fsg_edt_nearest_label", _p(d2), int(s is not None), len(cands), D * H * W, _p(cand_t), _p(k8), _p(out),
                      _stream())
    return out


def _quantile_linear(d, q):
    """torch.quantile(d, q) (linear interpolation) of a 1-D tensor of any length: torch.quantile itself up to its limit of
    metrics.QUANTILE_MAX_ELEMENTS, above it the same formula on a sort"""
    from . import metrics
    n = d.numel()
    if n <= metrics.QUANTILE_MAX_ELEMENTS:
        return torch.quantile(d, q)
    srt = torch.sort(d).values
    pos = q * (n - 1)
    lo = int(pos)
    hi = min(lo + 1, n - 1)
    return srt[lo] + (srt[hi] - srt[lo]) * (pos - lo)


def labelmap_distances(a, b, spacing=(1., 1., 1.)):
    """The symmetric surface-distance statistics between the voxel clouds of two label maps -- what the reference's
    `label_label_assd` (metrics.py:79-93) measures with open3d point-cloud distances -> (mean, std, hd, hd95), fp64 tensors on
    the device, each the average of the two directions (`metrics._symmetric_point_distances`).  a, b (D, H, W), bool or integer,
    nonzero = set; `spacing` in (x, y, z), as `mask_to_points` takes it.  The distance from a set voxel of `a` to the nearest
    set voxel of `b` is the distance transform of b == 0 read at that voxel (squared distances in fp32 as in
    `distance_transform_edt`, square roots and statistics in fp64).  An empty mask gives four NaNs (`metrics._nan4`).  Parity
    with open3d is unpinned; scipy's transform is the checker."""
    from . import metrics
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"labelmap_distances: expected two volumes (D, H, W) of one shape, got {tuple(a.shape)}, {tuple(b.shape)}")
    _need_gpu(a, b)
    sx, sy, sz = (float(v) for v in spacing)
    with torch.no_grad():
        am, bm = a != 0, b != 0
        if not bool(am.any()) or not bool(bm.any()):
            return metrics._nan4()
        d2 = distance_transform_edt(torch.stack((~bm, ~am)), sampling=(sz, sy, sx), squared=True)
        d_ab, d_ba = d2[0][am].double().sqrt_(), d2[1][bm].double().sqrt_()
        if max(d_ab.numel(), d_ba.numel()) <= metrics.QUANTILE_MAX_ELEMENTS:
            return metrics._symmetric_point_distances(d_ab, d_ba)
        both = (d_ab, d_ba)
        return (sum(d.mean() for d in both) / 2, sum(d.std() for d in both) / 2, sum(d.max() for d in both) / 2,
                sum(_quantile_linear(d, 0.95) for d in both) / 2)


# ------------------------------------------------------------------ voxel patch augmentation, resampling (csrc/spatial.hip)
BSPLINE_PAD = _lib.BSPLINE_PAD      # edge-replicated samples the prefilter adds on every side (scipy's own for mode='nearest')
ELASTIC_MAX_SIGMA = _lib.ELASTIC_MAX_SIGMA
_LABEL_KINDS = {torch.uint8: _lib.LABEL_U8, torch.int32: _lib.LABEL_I32, torch.int64: _lib.LABEL_I64}


def _volume5(t, what, floating=True):
    if t.dim() != 5 or t.numel() == 0 or (floating and not t.is_floating_point()):
        raise ValueError(f"{what}: expected a{' floating-point' if floating else 'n'} (B, C, D, H, W) tensor, got "
                         f"{tuple(t.shape)} {t.dtype}")
    if (t.shape[2] + 2 * BSPLINE_PAD) * (t.shape[3] + 2 * BSPLINE_PAD) * (t.shape[4] + 2 * BSPLINE_PAD) >= 2 ** 31:
        raise ValueError(f"{what}: volume {tuple(t.shape[2:])} holds 2^31 voxels or more with its padding")
    if t.shape[0] > 65535:
        raise ValueError(f"{what}: batch of {t.shape[0]} (at most 65535)")


def bspline_prefilter(vol):
    """vol (B, C, D, H, W) floating point -> the cubic B-spline coefficients (B, C, D + 24, H + 24, W + 24) fp32 of the volume
    extended by BSPLINE_PAD = 12 edge-replicated samples on every side: what scipy.ndimage.map_coordinates(order=3,
    mode='nearest') computes before it interpolates.  Three axis passes (csrc/spatial.hip).  Feed it to `spatial_transform(...,
    order_data=3, prefiltered=True)`; a data set keeps it across epochs."""
    _volume5(vol, "bspline_prefilter")
    _need_gpu(vol)
    x = _f32c(vol)
    B, C, D, H, W = x.shape
    p = 2 * BSPLINE_PAD
    dev = x.device
    with torch.no_grad(), torch.cuda.device(dev):
        a = torch.empty(B, C, D, H, W + p, dtype=torch.float32, device=dev)
        _lib.call("fsg_bspline_prefilter_axis_f32", _p(x), B * C * D * H, W, 1, _p(a), _stream())
        b = torch.empty(B, C, D, H + p, W + p, dtype=torch.float32, device=dev)
        _lib.call("fsg_bspline_prefilter_axis_f32", _p(a), B * C * D, H, W + p, _p(b), _stream())
        del a
        out = torch.empty(B, C, D + p, H + p, W + p, dtype=torch.float32, device=dev)
        _lib.call("fsg_bspline_prefilter_axis_f32", _p(b), B * C, D, (H + p) * (W + p), _p(out), _stream())
    return out


def _per_item(v, B, dev, what, lo=None, hi=None):
    """a number or a (B,) tensor -> (B,) fp32 on the device; a number is range-checked here, a tensor is not read"""
    if torch.is_tensor(v):
        if v.shape != (B,):
            raise ValueError(f"{what} must be a number or a tensor of shape ({B},), got {tuple(v.shape)}")
        _need_gpu(v)
        return _f32c(v)
    v = float(v)
    if (lo is not None and not v > lo) or (hi is not None and not v <= hi):
        raise ValueError(f"{what} = {v} must lie in ({lo}, {hi}]")
    return torch.full((B,), v, dtype=torch.float32, device=dev)


def elastic_field(noise, sigma, alpha):
    """noise (B, 3, pd, ph, pw) -> alpha * scipy.ndimage.gaussian_filter(noise, sigma, mode='constant', cval=0, truncate=4)
    per item and component, fp32: batchgenerators' elastic displacement field (`elastic_deform_coordinates`).  sigma, alpha: a
    number or a (B,) device tensor (never read on the host).  scipy's taps, radius int(4 sigma + 0.5), which may exceed an
    axis; one launch per axis for all items and components.  sigma must lie in (0, 255]; an item of a sigma TENSOR that does
    not gives NaN."""
    if noise.dim() != 5 or noise.shape[1] != 3 or noise.numel() == 0 or not noise.is_floating_point():
        raise ValueError(f"elastic_field: expected floating-point noise (B, 3, pd, ph, pw), got {tuple(noise.shape)} {noise.dtype}")
    B, _, pd, ph, pw = noise.shape
    if 3 * pd * ph * pw >= 2 ** 31 or B > 65535:
        raise ValueError(f"elastic_field: field {tuple(noise.shape)}: 2^31 values or more per item, or more than 65535 items")
    dev = noise.device
    sg = _per_item(sigma, B, dev, "elastic_field: sigma", 0.0, ELASTIC_MAX_SIGMA)
    al = _per_item(alpha, B, dev, "elastic_field: alpha")
    _need_gpu(noise)
    x = _f32c(noise)
    with torch.no_grad(), torch.cuda.device(dev):
        out, tmp = torch.empty_like(x), torch.empty_like(x)
        _lib.call("fsg_gauss_axis_f32", _p(x), B, 3 * pd * ph, pw, 1, _p(sg), None, _p(out), _stream())
        _lib.call("fsg_gauss_axis_f32", _p(out), B, 3 * pd, ph, pw, _p(sg), None, _p(tmp), _stream())
        _lib.call("fsg_gauss_axis_f32", _p(tmp), B, 3, pd, ph * pw, _p(sg), _p(al), _p(out), _stream())
    return out


def _patch3(patch_size, what):
    try:
        p = tuple(int(v) for v in patch_size)
    except TypeError:
        p = ()
    if len(p) != 3 or min(p) < 1 or p[0] * p[1] * p[2] >= 2 ** 31:
        raise ValueError(f"{what}: patch_size must be three positive integers (pd, ph, pw) with fewer than 2^31 voxels, got "
                         f"{patch_size!r}")
    return p


def spatial_transform(img, seg, patch_size, matrix, centre, elastic=None, mirror=None, order_data=3, order_seg=0,
                      prefiltered=False, intensity=None):
    """One fused launch (csrc/spatial.hip) that cuts a transformed patch out of an image and its label map: for output voxel o
    of item b the source coordinate is  matrix_b @ ((o - (patch_size - 1) / 2) + elastic_b(o)) + centre_b,  in voxel units, axes
    (D, H, W) -> (img_patch (B, C, *patch_size) fp32, seg_patch (B, Cs, *patch_size) int64); either input may be None (its
    output is then None).

    img (B, C, D, H, W) floating point, read at order_data 3 (cubic B-spline; the coefficients come from `bspline_prefilter`,
      or are `img` itself, (B, C, D + 24, H + 24, W + 24), with prefiltered=True), 1 (trilinear) or 0 (nearest).  Borders:
      edge replication -- orders 0 and 1 clamp the coordinate to [0, n - 1]; order 3 evaluates the spline in the 12 padded
      samples and runs into the edge coefficient beyond them, as scipy's map_coordinates(mode='nearest') does.
    seg (B, Cs, D, H, W) integer (values must fit an int32): order_seg 0 = nearest (floor(x + 0.5)), 1 = batchgenerators'
      per-label rule (the largest label whose summed trilinear weight is >= 0.5, else 0).  A coordinate outside [0, n - 1] on
      any axis gives 0 (scipy's mode='constant', cval=0).
    matrix (B, 3, 3), centre (B, 3), elastic (B, 3, *patch_size) or None, mirror (B, 3) bool or None (a set flag reverses the
      item's OUTPUT along that axis, after everything else), intensity (a, b) or None: img_patch = a * value + b.
    No host read, no atomics: bit-reproducible, batch-independent, capturable in a graph."""
    what = "spatial_transform"
    pd, ph, pw = _patch3(patch_size, what)
    if img is None and seg is None:
        raise ValueError(f"{what}: neither an image nor a label map")
    if order_data not in (0, 1, 3) or order_seg not in (0, 1):
        raise ValueError(f"{what}: order_data must be 0, 1 or 3 and order_seg 0 or 1, got {order_data!r}, {order_seg!r}")
    if prefiltered and (order_data != 3 or img is None):
        raise ValueError(f"{what}: prefiltered=True goes with an image and order_data=3")
    pad = BSPLINE_PAD if prefiltered else 0
    shape = None
    if img is not None:
        _volume5(img, f"{what}: img")
        if min(img.shape[2:]) <= 2 * pad:
            raise ValueError(f"{what}: prefiltered coefficients {tuple(img.shape)} are smaller than their padding")
        shape = (img.shape[0],) + tuple(s - 2 * pad for s in img.shape[2:])
    if seg is not None:
        _volume5(seg, f"{what}: seg", floating=False)
        if seg.is_floating_point() or seg.is_complex() or seg.dtype == torch.bool:
            raise ValueError(f"{what}: seg must be an integer tensor, got {seg.dtype}")
        sshape = (seg.shape[0],) + tuple(seg.shape[2:])
        if shape is not None and sshape != shape:
            raise ValueError(f"{what}: img {tuple(img.shape)} (padding {pad}) and seg {tuple(seg.shape)} do not match")
        shape = sshape
    B, D, H, W = shape
    if not torch.is_tensor(matrix) or not torch.is_tensor(centre) or matrix.shape != (B, 3, 3) or centre.shape != (B, 3):
        raise ValueError(f"{what}: matrix must be a ({B}, 3, 3) tensor and centre ({B}, 3)")
    if elastic is not None and elastic.shape != (B, 3, pd, ph, pw):
        raise ValueError(f"{what}: elastic must be ({B}, 3, {pd}, {ph}, {pw}), got {tuple(elastic.shape)}")
    if mirror is not None and (mirror.shape != (B, 3) or mirror.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"{what}: mirror must be a bool or uint8 tensor of shape ({B}, 3)")
    ia, ib = (1.0, 0.0) if intensity is None else (float(intensity[0]), float(intensity[1]))
    _need_gpu(img, seg, matrix, centre, elastic, mirror)
    dev = matrix.device
    with torch.no_grad():
        src, C, out_img = None, 0, None
        if img is not None:
            src = bspline_prefilter(img) if order_data == 3 and not prefiltered else _f32c(img)
            C = src.shape[1]
            out_img = torch.empty(B, C, pd, ph, pw, dtype=torch.float32, device=dev)
        lab, Cs, kind, out_seg = None, 0, 0, None
        if seg is not None:
            lab = seg.contiguous() if seg.dtype in _LABEL_KINDS else seg.to(torch.int32).contiguous()
            Cs, kind = lab.shape[1], _LABEL_KINDS[lab.dtype]
            out_seg = torch.empty(B, Cs, pd, ph, pw, dtype=torch.int64, device=dev)
        m, c = _f32c(matrix), _f32c(centre)
        e = None if elastic is None else _f32c(elastic)
        f = None if mirror is None else mirror.contiguous().view(torch.uint8)
        with torch.cuda.device(dev):
            _lib.call("fsg_spatial_resample_f32", _p(src), C, order_data, _p(lab), kind, Cs, order_seg, B, D, H, W, pd, ph, pw,
                      _p(m), _p(c), _p(e), _p(f), ia, ib, _p(out_img), _p(out_seg), _stream())
    return out_img, out_seg


# ------------------------------------------------------------------ point cloud <-> dense grid, spectral PSR (csrc/grid_points.hip)
GRID_MODES = {"torch": _lib.GRID_TORCH, "sap": _lib.GRID_SAP}


def _grid_mode(mode):
    if isinstance(mode, str) and mode.lower() in GRID_MODES:
        return GRID_MODES[mode.lower()]
    raise ValueError(f"mode must be 'torch' (grid_sample's convention) or 'sap' (point_rasterize's), got {mode!r}")


def _grid_size(size, m):
    try:
        size = tuple(int(s) for s in size)
    except TypeError:
        size = ()
    if len(size) != 3 or min(size) < (2 if m == _lib.GRID_SAP else 1) or size[0] * size[1] * size[2] >= 2 ** 31 - 1:
        raise ValueError(f"grid size must be three positive integers (D, H, W) with D H W < 2^31 - 1, each >= 2 in 'sap' mode; "
                         f"got {size}")
    return size


def _grid_check(first, coords, what, first_dims):
    """the shared checks of splat and sample: `first` is values (B, C, N) or grid (B, C, D, H, W), coords (B, N, 3)"""
    for t, name in ((first, what), (coords, "coords")):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if first.dim() != first_dims or first.shape[1] < 1 or first.shape[0] < 1:
        raise ValueError(f"expected {what} with {first_dims} dimensions and B, C >= 1, got {tuple(first.shape)}")
    if coords.dim() != 3 or coords.shape[2] != 3 or coords.shape[0] != first.shape[0]:
        raise ValueError(f"expected coords (B, N, 3) with B = {first.shape[0]}, got {tuple(coords.shape)}")
    if first.device != coords.device:
        raise ValueError(f"{what} and coords are on different devices ({first.device}, {coords.device})")
    if first.shape[0] > 65535:
        raise ValueError(f"at most 65535 items per call, got {first.shape[0]}")


def _splat_raw(values, coords, size, m):
    """values (B, C, N), coords (B, N, 3), both fp32 and contiguous (the callers convert with _f32c) -> grid (B, C, D, H, W):
    corners, a stable sort per item, the sums"""
    B, C, N = values.shape
    D, H, W = size
    if N == 0:
        return torch.zeros(B, C, D, H, W, dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        keys = torch.empty(B, 8 * N, dtype=torch.int32, device=values.device)
        w = torch.empty(B, 8 * N, dtype=torch.float32, device=values.device)
        _lib.call("fsg_grid_corners_f32", _p(coords), B, N, D, H, W, m, _p(keys), _p(w), _stream())
        skeys, perm = torch.sort(keys, dim=1, stable=True)
        grid = torch.empty(B, C, D, H, W, dtype=torch.float32, device=values.device)
        ws = _lib.workspace("fsg_grid_splat", B, C, N, device=values.device)
        _lib.call("fsg_grid_splat_sorted_f32", _p(values), _p(skeys), _p(perm), _p(w), B, C, N, D, H, W, _p(grid), _p(ws),
                  ws.numel(), _stream())
    return grid


def _sample_raw(grid, coords, weights, m, want_sampled=True):
    """grid (B, C, D, H, W), coords (B, N, 3), weights (B, C, N) or None, all fp32 and contiguous -> (sampled (B, C, N) or None,
    grad_coords or None)"""
    B, C, D, H, W = grid.shape
    N = coords.shape[1]
    sampled = torch.empty(B, C, N, dtype=torch.float32, device=grid.device) if want_sampled else None
    gc = torch.empty(B, N, 3, dtype=torch.float32, device=grid.device) if weights is not None else None
    if N > 0:
        with torch.cuda.device(grid.device):
            _lib.call("fsg_grid_sample_f32", _p(grid), _p(coords), _p(weights), B, C, N, D, H, W, m, _p(sampled), _p(gc),
                      _stream())
    return sampled, gc


class _Splat(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, values, coords, size, m):
        values, coords = _f32c(values), _f32c(coords)          # the kernels read fp32: any other floating type is converted
        ctx.save_for_backward(values, coords)
        ctx.m = m
        return _splat_raw(values, coords, size, m)

    @staticmethod
    @_amp_bwd
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        values, coords = ctx.saved_tensors
        need_v, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_v or need_c):
            return None, None, None, None
        gv, gc = _sample_raw(_f32c(g), coords, values if need_c else None, ctx.m, want_sampled=need_v)
        return gv, gc, None, None


class _Sample(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, grid, coords, m):
        grid, coords = _f32c(grid), _f32c(coords)
        ctx.save_for_backward(grid, coords)
        ctx.m = m
        return _sample_raw(grid, coords, None, m)[0]

    @staticmethod
    @_amp_bwd
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        grid, coords = ctx.saved_tensors
        g = _f32c(g)
        gg = _splat_raw(g, coords, tuple(grid.shape[2:]), ctx.m) if ctx.needs_input_grad[0] else None
        gc = _sample_raw(grid, coords, g, ctx.m, want_sampled=False)[1] if ctx.needs_input_grad[1] else None
        return gg, gc, None


def splat_to_grid(values, coords, size, mode):
    """values (B, C, N) at coords (B, N, 3) -> grid (B, C, D, H, W), size = (D, H, W): the sum of the points' trilinear
    contributions.  mode 'torch': coords (x -> W, y -> H, z -> D) in [-1, 1], the exact adjoint of F.grid_sample(mode='bilinear',
    padding_mode='zeros', align_corners=False) (models/divroc.py:24-42); mode 'sap': coords (0 -> D, 1 -> H, 2 -> W) in [0, 1],
    models/dpsr_utils.py:227-287 (point_rasterize).  Any floating-point input is converted to fp32, the result is fp32.
    Gradients to values and coords (one gather launch); no double backward.
    No floating-point atomics: the same input gives the same bits, an item gives the same bits alone and in a batch."""
    m = _grid_mode(mode)
    size = _grid_size(size, m)
    _grid_check(values, coords, "values", 3)
    if values.shape[2] != coords.shape[1]:
        raise ValueError(f"values {tuple(values.shape)} and coords {tuple(coords.shape)} disagree about the number of points")
    _need_gpu(values, coords)
    return _Splat.apply(values, coords, size, m)


def sample_grid(grid, coords, mode):
    """grid (B, C, D, H, W) read at coords (B, N, 3) -> (B, C, N), trilinear, in the convention of `mode` (see splat_to_grid):
    'torch' is F.grid_sample(..., align_corners=False, padding_mode='zeros'), 'sap' is models/dpsr_utils.py:156-199
    (grid_interp).  Gradients to grid (a splat) and to coords (indices constant, torch's convention); no double backward."""
    m = _grid_mode(mode)
    _grid_check(grid, coords, "grid", 5)
    _grid_size(grid.shape[2:], m)
    _need_gpu(grid, coords)
    return _Sample.apply(grid, coords, m)


def _psr_raw(x, res, sig, adjoint):
    B = x.shape[0]
    R0, R1, R2 = res
    out = torch.empty((B, R0, R1, R2 // 2 + 1) if not adjoint else (B, 3, R0, R1, R2 // 2 + 1), dtype=torch.complex64,
                      device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("fsg_psr_spectral_f32", _p(x), B, R0, R1, R2, float(sig), int(adjoint), _p(out), _stream())
    return out


class _PSRSolve(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, nhat, res, sig):
        ctx.res, ctx.sig = res, sig
        return _psr_raw(nhat.contiguous(), res, sig, False)

    @staticmethod
    @_amp_bwd
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _psr_raw(g.to(torch.complex64).contiguous(), ctx.res, ctx.sig, True), None, None


def psr_spectral_solve(normal_field_hat, res, sig):
    """models/dpsr_net.py:74-87 in one launch: normal_field_hat (B, 3, R0, R1, R2 / 2 + 1) complex64 = rfftn of the rasterised
    normals over res = (R0, R1, R2) -> Phi (B, R0, R1, R2 / 2 + 1) complex64 = the Gaussian filter (sig), the divergence, the
    division by the Laplacian and the zeroed DC term; irfftn(Phi, s=res) is the indicator grid.  The backward is the adjoint on
    the same kernel."""
    try:
        res = tuple(int(r) for r in res)
    except TypeError:
        res = ()
    if len(res) != 3 or min(res) < 1:
        raise ValueError(f"res must be three positive integers, got {res}")
    if not torch.is_tensor(normal_field_hat) or normal_field_hat.dtype != torch.complex64:
        raise TypeError("normal_field_hat must be a complex64 tensor (torch.fft.rfftn of an fp32 field)")
    want = (3, res[0], res[1], res[2] // 2 + 1)
    if normal_field_hat.dim() != 5 or tuple(normal_field_hat.shape[1:]) != want or normal_field_hat.shape[0] < 1:
        raise ValueError(f"expected normal_field_hat (B, {', '.join(map(str, want))}) for res {res}, got "
                         f"{tuple(normal_field_hat.shape)}")
    if not float(sig) >= 0:
        raise ValueError(f"sig must be >= 0, got {sig}")
    _need_gpu(normal_field_hat)
    return _PSRSolve.apply(normal_field_hat, res, float(sig))


# ------------------------------------------------------------------ marching cubes (csrc/marching_cubes.hip)
def _mc_mask(mask, shape, what):
    """mask or None -> (uint8 contiguous or None, item stride); a mask has the volume's shape, or (D, H, W) shared by all items"""
    if mask is None:
        return None, 0
    if not torch.is_tensor(mask) or mask.is_floating_point() or tuple(mask.shape) not in (tuple(shape), tuple(shape[1:])):
        raise ValueError(f"{what}: mask must be a bool or integer tensor of shape {tuple(shape)} or {tuple(shape[1:])}, got "
                         f"{tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    m = (mask != 0).to(torch.uint8).contiguous()
    return m, (0 if mask.dim() == 3 else shape[1] * shape[2] * shape[3])


def _mc_shape(shape, what):
    B, D, H, W = shape
    if B < 1 or min(D, H, W) < 2 or B > 65535 or B * D * H * W >= 2 ** 31:
        raise ValueError(f"{what}: need B in 1..65535, every grid size >= 2 and B D H W < 2^31, got {tuple(shape)}")


def _mc_run(count, emit, shape, dev, local, spacing):
    """count (four launches), the one host read that sizes the outputs, emit (three launches).  count(ws, nbytes, totals) and
    emit(local, sx, sy, sz, ws, nbytes, totals, nv, nf, verts, faces, normals) bind the volume."""
    B, D, H, W = shape
    with torch.cuda.device(dev):
        ws = _lib.workspace("fsg_mc", B, D, H, W, device=dev)
        nbytes = ws.numel()
        totals = torch.empty(4 * B + 1, dtype=torch.int64, device=dev)
        count(ws, nbytes, totals)
        host = totals[:2 * B + 1].tolist()                 # the readback: the result's size depends on the data
        num_verts, num_faces, flag = host[0:2 * B:2], host[1:2 * B:2], host[2 * B]
        if max(num_verts + num_faces) >= 2 ** 31:
            raise ValueError("marching_cubes: an item has 2^31 or more vertices or faces")
        nv, nf = sum(num_verts), sum(num_faces)
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf, 3, dtype=torch.int64, device=dev)
        normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        if flag == 0 and nv > 0:
            emit(int(bool(local)), float(spacing[0]), float(spacing[1]), float(spacing[2]), ws, nbytes, totals, nv, nf, verts, faces,
                 normals)
    return verts, faces, normals, num_verts, num_faces, flag


def marching_cubes(field, isolevel=0.0, return_local_coords=True, mask=None, validate=True):
    """pytorch3d.ops.marching_cubes (models/dpsr_utils.py:60-61) with the vertex normals of Meshes.verts_normals_packed, on our
    own case table (fissure_segmentation_amd/_mc_table.py; parity with pytorch3d is unpinned).  field (B, D, H, W), any
    floating type (converted to fp32), every size >= 2 -> packed
      verts (sum V, 3) fp32, columns (x, y, z) = position along (W, H, D): in [-1, 1] with return_local_coords (node i of an axis
        of S nodes is 2 i / (S - 1) - 1), else in index units; one per grid edge that crosses the isolevel, ordered by
        (item, z, y, x, axis) of the edge's lower node
      faces (sum F, 3) int64, indices LOCAL to their item, ordered by (item, cell, table order)
      normals (sum V, 3) fp32: the faces' (v1 - v0) x (v2 - v0) summed per vertex and divided by max(|n|, 1e-6); they point
        toward increasing values
      num_verts, num_faces: lists of B ints.
    A node is inside iff value < isolevel.  mask (bool / integer, the field's shape or (D, H, W)): a cell emits iff its 8 nodes
    are in the mask, and only vertices of emitting cells exist (this rule is ours).  validate=True raises ValueError on a
    non-finite value (the flag rides on the count readback).  An item without a crossing has 0 vertices and faces.  The call reads
    the totals back to size its outputs, so it cannot be captured into a graph.  No gradient: models/dpsr_utils.py's
    DifferentiableMarchingCubes supplies the reference's.  Deterministic: the same input gives the same bits, alone or in a batch."""
    if not torch.is_tensor(field) or not field.is_floating_point():
        raise TypeError(f"field must be a floating-point tensor, got {field.dtype if torch.is_tensor(field) else type(field).__name__}")
    if field.dim() != 4:
        raise ValueError(f"marching_cubes: expected field (B, D, H, W), got {tuple(field.shape)}")
    _mc_shape(field.shape, "marching_cubes")
    m, mstride = _mc_mask(mask, field.shape, "marching_cubes")
    iso = float(isolevel)
    if iso != iso or iso in (float("inf"), float("-inf")):
        raise ValueError(f"isolevel must be finite, got {isolevel!r}")
    _need_gpu(field, m)
    if m is not None and m.device != field.device:
        raise ValueError(f"field and mask are on different devices ({field.device}, {m.device})")
    f = _f32c(field)
    B, D, H, W = f.shape

    def count(ws, nbytes, totals):
        _lib.call("fsg_mc_count_f32", _p(f), _p(m), mstride, B, D, H, W, iso, int(bool(validate)), _p(ws), nbytes, _p(totals),
                  _stream())

    def emit(local, sx, sy, sz, ws, nbytes, totals, nv, nf, verts, faces, normals):
        _lib.call("fsg_mc_emit_f32", _p(f), B, D, H, W, iso, local, sx, sy, sz, _p(ws), nbytes, _p(totals), nv, nf, _p(verts),
                  _p(faces), _p(normals), _stream())

    with torch.no_grad():
        verts, faces, normals, num_verts, num_faces, flag = _mc_run(count, emit, f.shape, f.device, return_local_coords, (1, 1, 1))
    if flag:
        raise ValueError("marching_cubes: the field holds a non-finite value (validate=False meshes it as it is: NaN is outside)")
    return verts, faces, normals, num_verts, num_faces


def marching_cubes_labels(labels, first_label, num_labels, spacing=(1, 1, 1), mask=None):
    """One surface per label of ONE integer volume, in one batched call: labels (D, H, W), item b = the object
    labels == first_label + b, meshed as the field (labels != first_label + b) at level 0.5 (every vertex is an edge midpoint,
    normals point out of the object).  Vertices are in index units times spacing = (sx, sy, sz) for the (x, y, z) columns.  mask
    (D, H, W) as in `marching_cubes`.  -> verts, faces, normals, num_verts, num_faces as `marching_cubes` returns them."""
    if not torch.is_tensor(labels) or labels.is_floating_point() or labels.dim() != 3:
        raise ValueError(f"marching_cubes_labels: expected an integer label volume (D, H, W), got "
                         f"{(tuple(labels.shape), labels.dtype) if torch.is_tensor(labels) else type(labels).__name__}")
    B = int(num_labels)
    shape = (B,) + tuple(labels.shape)
    _mc_shape(shape, "marching_cubes_labels")
    try:
        spacing = tuple(float(s) for s in spacing)
    except TypeError:
        spacing = ()
    if len(spacing) != 3 or not all(0 < s < float("inf") for s in spacing):
        raise ValueError(f"spacing must be three positive numbers (sx, sy, sz), got {spacing}")
    if mask is not None and torch.is_tensor(mask) and mask.dim() != 3:
        raise ValueError(f"marching_cubes_labels: the mask is shared by all labels, expected (D, H, W), got {tuple(mask.shape)}")
    m, _ = _mc_mask(mask, shape, "marching_cubes_labels")
    _need_gpu(labels, m)
    if m is not None and m.device != labels.device:
        raise ValueError(f"labels and mask are on different devices ({labels.device}, {m.device})")
    lab = labels.to(torch.int32).contiguous()
    first = int(first_label)
    _, D, H, W = shape

    def count(ws, nbytes, totals):
        _lib.call("fsg_mc_count_labels_i32", _p(lab), _p(m), 0, first, B, D, H, W, _p(ws), nbytes, _p(totals), _stream())

    def emit(local, sx, sy, sz, ws, nbytes, totals, nv, nf, verts, faces, normals):
        _lib.call("fsg_mc_emit_labels_i32", _p(lab), first, B, D, H, W, local, sx, sy, sz, _p(ws), nbytes, _p(totals), nv, nf,
                  _p(verts), _p(faces), _p(normals), _stream())

    with torch.no_grad():
        return _mc_run(count, emit, shape, lab.device, False, spacing)[:5]


# ------------------------------------------------------------------ surface fitting: orientation, mesh clean-up (csrc/mesh_cleanup.hip)
def orient_normals_consistent(xyz, normals, offset, k, idx=None):
    """Globally consistent signs for the normals of a packed cloud (fsg_orient_normals_f32), what open3d's
    orient_normals_consistent_tangent_plane does for data_processing/surface_fitting.py:64.

    xyz, normals (n, 3), offset (b,) cumulative segment ends, 2 <= k <= 64; idx (n, k): neighbour lists in knn_segment's layout
    (self first), built here when None.  Per segment the graph {u, idx[u, j]}, 1 <= j < min(k, n_s - 1), weighted by
    1 - |n_u . n_v|, gets its minimum spanning forest (Boruvka rounds on the device) and the signs are carried along it.  Per
    connected component the member of largest z (lowest index on ties) ends with n_z >= 0.  The graph is NOT connected by extra
    Euclidean edges as open3d does: every component is oriented on its own.
    -> oriented (n, 3) fp32 = normals with the sign flipped or not, signs (n,) int8 (+1 / -1), component (n,) int32: the smallest
    member of the point's component.  No host read; bitwise reproducible; a segment gives the same bits alone and in a batch.
    At most 2^20 points per call.  Not differentiable."""
    k = _neighborhood_size(k)
    if not torch.is_tensor(xyz) or not xyz.is_floating_point() or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"expected packed points xyz (n, 3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if not torch.is_tensor(normals) or not normals.is_floating_point() or normals.shape != xyz.shape:
        raise ValueError(f"normals must be a floating-point tensor of the shape of xyz {tuple(xyz.shape)}")
    if not torch.is_tensor(offset) or offset.is_floating_point() or offset.dim() != 1 or offset.shape[0] < 1:
        raise ValueError("offset must be a 1-D integer tensor of cumulative segment ends")
    n = xyz.shape[0]
    if n > _lib.ORIENT_MAX_POINTS:
        raise ValueError(f"orient_normals_consistent: {n} points, at most {_lib.ORIENT_MAX_POINTS} per call (20 bits per endpoint "
                         f"in the edge key)")
    _need_gpu(xyz, normals, offset, idx)
    with torch.no_grad():
        x, nr, off = _f32c(xyz), _f32c(normals), offset.to(torch.int32).contiguous()
        dev = x.device
        out = torch.empty(n, 3, dtype=torch.float32, device=dev)
        signs = torch.empty(n, dtype=torch.int8, device=dev)
        comp = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return out, signs, comp
        if idx is None:
            idx = knn_segment(k, x, x, off, off)[0]
        else:
            if not torch.is_tensor(idx) or idx.is_floating_point() or idx.dtype == torch.bool or tuple(idx.shape) != (n, k):
                raise ValueError(f"idx must be an integer tensor of shape ({n}, {k}): knn_segment's lists")
            idx = idx.to(torch.int32).contiguous()
        with torch.cuda.device(dev):
            ws = _lib.workspace("fsg_orient_normals", n, k, device=dev)
            _lib.call("fsg_orient_normals_f32", _p(x), _p(nr), _p(idx), _p(off), off.shape[0], n, k, _p(ws), ws.numel(), _p(out),
                      _p(signs), _p(comp), _stream())
    return out, signs, comp


class _PackedMeshes:
    """the meshes of one call packed for csrc/mesh_cleanup.hip: verts (V, 3) fp32, faces (F, 3) int32 into verts, normals or None,
    the first vertex / face of every mesh as host lists and as int32 / int64 device tensors (B + 1), the mesh of every face"""

    def __init__(self, who, meshes):
        if hasattr(meshes, "verts_list") and hasattr(meshes, "faces_list"):
            vl, fl = meshes.verts_list(), meshes.faces_list()
            nl = meshes.verts_normals_list() if getattr(meshes, "_normals", None) is not None else None
        elif isinstance(meshes, (tuple, list)) and len(meshes) == 2 and torch.is_tensor(meshes[0]) and torch.is_tensor(meshes[1]):
            vl, fl, nl = [meshes[0]], [meshes[1]], None
        else:
            raise TypeError(f"{who}: expected fissure_segmentation_amd.mesh.Meshes or one (verts, faces) pair, got "
                            f"{type(meshes).__name__}")
        if not vl:
            raise ValueError(f"{who}: empty batch of meshes")
        for m, (v, f) in enumerate(zip(vl, fl)):
            if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or not v.is_floating_point():
                raise ValueError(f"{who}: mesh {m}: expected verts (V,3) and faces (F,3), got {tuple(v.shape)} and {tuple(f.shape)}")
            if f.is_floating_point() or f.dtype == torch.bool:
                raise ValueError(f"{who}: mesh {m}: faces must hold integer vertex indices, got {f.dtype}")
        _need_gpu(*vl, *fl)
        self.B, self.dev = len(vl), vl[0].device
        self.nv, self.nf = [v.shape[0] for v in vl], [f.shape[0] for f in fl]
        self.voff, self.foff = [0], [0]
        for a, b in zip(self.nv, self.nf):
            self.voff.append(self.voff[-1] + a)
            self.foff.append(self.foff[-1] + b)
        self.V, self.F = self.voff[-1], self.foff[-1]
        if max(self.V, 3 * self.F) >= 2 ** 31:
            raise ValueError(f"{who}: the batch has 2^31 or more vertices or half-edges")
        self.verts = torch.cat([_f32c(v) for v in vl])
        self.faces = torch.cat([f.detach().to(torch.int32) + b for f, b in zip(fl, self.voff)]).contiguous()
        self.normals = None if nl is None else torch.cat([_f32c(x) for x in nl])
        self.voff_t = torch.tensor(self.voff, dtype=torch.int32).to(self.dev)
        self.foff_t = torch.tensor(self.foff, dtype=torch.int64).to(self.dev)
        self.face_mesh = torch.repeat_interleave(torch.arange(self.B, device=self.dev), torch.tensor(self.nf).to(self.dev),
                                                 output_size=self.F)


def _face_components(pk):
    """-> clusters (F,) int32 local to the mesh, counts (B,) int64, both on the device; no host read"""
    dev, F = pk.dev, pk.F
    if F == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(pk.B, dtype=torch.int64, device=dev)
    f = pk.faces.long()
    a, b = f, f.roll(-1, 1)                                                  # half-edge 3 f + e = (f[e], f[e + 1])
    keys, half_edge = torch.sort((torch.minimum(a, b) * pk.V + torch.maximum(a, b)).reshape(-1))
    parent = torch.empty(F, dtype=torch.int32, device=dev)
    root = torch.empty(F, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fsg_face_union_i32", _p(keys), _p(half_edge), F, _p(parent), _p(root), _stream())
    is_root = (root == torch.arange(F, dtype=torch.int32, device=dev)).long()
    before = torch.cumsum(is_root, 0)                                        # roots up to and including f
    before = torch.cat([before.new_zeros(1), before])                        # [f]: roots before face f
    start = before[pk.foff_t]                                                # roots before the first face of every mesh
    clusters = (before[root.long()] - start[pk.face_mesh]).to(torch.int32)
    return clusters, start[1:] - start[:-1]


def mesh_face_components(meshes):
    """Edge-connected components of the triangles of a batch of meshes (fsg_face_union_i32), open3d's cluster_connected_triangles
    as utils/general_utils.py:177 calls it: two faces are adjacent iff they share an edge (the same unordered vertex pair);
    sharing only a vertex does not connect them, and an edge with more than two faces links all of them.

    meshes: `mesh.Meshes` or one (verts, faces) pair -> clusters (sum F,) int32, the cluster of every face within ITS mesh, the
    clusters of a mesh numbered 0 .. c - 1 in ascending order of their smallest face; counts (B,) int64 on the device.  The 3F
    edge keys are paired by torch.sort, the union is the kernel, the numbering a prefix sum.  No host read."""
    with torch.no_grad():
        return _face_components(_PackedMeshes("mesh_face_components", meshes))


def _check_clusters(who, pk, clusters):
    if not torch.is_tensor(clusters) or clusters.is_floating_point() or clusters.dtype == torch.bool or tuple(clusters.shape) != (pk.F,):
        raise ValueError(f"{who}: clusters must be an integer tensor of shape ({pk.F},), one entry per face of the batch")
    _need_gpu(clusters)
    return clusters.to(torch.int32)


def mesh_component_stats(meshes, clusters):
    """Area, number of distinct vertices and their coordinate sum for every face cluster of a batch (fsg_cluster_stats_f64), what
    utils/general_utils.py:177-195 takes from open3d's cluster_area and np.unique / np.mean.

    clusters (sum F,): `mesh_face_components`' numbers.  -> area (C,) fp64, num_verts (C,) int64, vert_sum (C, 3) fp64 with the
    clusters of mesh 0 first, then mesh 1's, ..., and counts: a list of B ints (C = their sum; one host read).  A vertex that two
    clusters touch counts in both.  Sums are fp64 in a fixed order: bitwise reproducible."""
    with torch.no_grad():
        pk = _PackedMeshes("mesh_component_stats", meshes)
        cl = _check_clusters("mesh_component_stats", pk, clusters)
        dev = pk.dev
        if pk.F == 0:
            return (torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                    torch.zeros(0, 3, dtype=torch.float64, device=dev), [0] * pk.B)
        # clusters per mesh = 1 + the largest number: a padded (B, max F) table and a row maximum (a scatter-max would send every
        # face's atomic to one of B addresses)
        table = torch.full((pk.B, max(pk.nf)), -1, dtype=torch.int64, device=dev)
        table[pk.face_mesh, torch.arange(pk.F, device=dev) - pk.foff_t[pk.face_mesh]] = cl.long()
        per_mesh = table.amax(1) + 1
        first = torch.cumsum(per_mesh, 0) - per_mesh
        host = torch.cat([per_mesh, cl.min().long().view(1)]).tolist()      # the readback: C sizes the outputs
        counts, C = host[:pk.B], sum(host[:pk.B])
        if host[pk.B] < 0:
            raise ValueError("mesh_component_stats: negative cluster number")
        glob = (cl.long() + first[pk.face_mesh]).to(torch.int32)
        sorted_cl, order = torch.sort(glob, stable=True)
        vkeys = torch.sort((glob.long()[:, None] * pk.V + pk.faces.long()).reshape(-1))[0]
        area = torch.empty(C, dtype=torch.float64, device=dev)
        nvert = torch.empty(C, dtype=torch.int64, device=dev)
        vsum = torch.empty(C, 3, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_cluster_stats_f64", _p(pk.verts), _p(pk.faces), _p(sorted_cl), _p(order), _p(vkeys), pk.V, pk.F, C, _p(area),
                      _p(nvert), _p(vsum), _stream())
    return area, nvert, vsum, counts


def mesh_remove_vertices(meshes, keep=None, box=None, mask=None, spacing=None, face_keep=None, drop_unreferenced=False):
    """Remove vertices (and the faces that lose one) from a batch of meshes and compact it (fsg_mesh_keep_flags_u8,
    fsg_mesh_face_flags_u8, fsg_mesh_compact_f32): open3d's remove_vertices_by_mask / crop / remove_triangles_by_mask /
    remove_unreferenced_vertices as utils/general_utils.py:157-209 and data_processing/surface_fitting.py:71-82 use them.

    A vertex is kept iff all the given tests pass: keep (sum V,) bool; box (2, 3) for all meshes or (B, 2, 3), rows (lo, hi) in
    (x, y, z), inclusive; mask (D, H, W) bool with spacing (sx, sy, sz): mask[iz, iy, ix] at i = floor(v / spacing), indices
    clamped from above like the reference's, a NEGATIVE index counts as outside (the reference's indexing wraps it around).
    A face survives iff its three vertices do and face_keep (sum F,) bool, if given, is set.  drop_unreferenced also removes the
    vertices that no surviving face names.  Survivors keep their order, faces are re-indexed.
    -> `mesh.Meshes` of as many meshes (vertex normals carried along when the input has them).  One host read (the sizes)."""
    from .mesh import Meshes
    with torch.no_grad():
        pk = _PackedMeshes("mesh_remove_vertices", meshes)
        dev, V, F, B = pk.dev, pk.V, pk.F, pk.B

        def flags(t, n, what):
            if t is None:
                return None
            if not torch.is_tensor(t) or tuple(t.shape) != (n,) or t.is_floating_point():
                raise ValueError(f"mesh_remove_vertices: {what} must be a bool or integer tensor of shape ({n},)")
            _need_gpu(t)
            return (t != 0).to(torch.uint8).contiguous()
        keep, face_keep = flags(keep, V, "keep"), flags(face_keep, F, "face_keep")
        boxes = None
        if box is not None:
            boxes = torch.as_tensor(box, dtype=torch.float32).to(dev)
            if tuple(boxes.shape) == (2, 3):
                boxes = boxes.expand(B, 2, 3)
            if tuple(boxes.shape) != (B, 2, 3):
                raise ValueError(f"mesh_remove_vertices: box must be (2, 3) or ({B}, 2, 3): rows (lo, hi), got {tuple(boxes.shape)}")
            boxes = boxes.reshape(B, 6).contiguous()
        D = H = W = 0
        sp = (1., 1., 1.)
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dim() != 3 or mask.is_floating_point():
                raise ValueError("mesh_remove_vertices: mask must be a bool or integer tensor (D, H, W)")
            if spacing is None:
                raise ValueError("mesh_remove_vertices: a mask needs its spacing (sx, sy, sz)")
            sp = tuple(float(s) for s in (spacing.tolist() if torch.is_tensor(spacing) else spacing))
            if len(sp) != 3 or not all(0 < s < float("inf") for s in sp):
                raise ValueError(f"mesh_remove_vertices: spacing must be three positive numbers (sx, sy, sz), got {sp}")
            _need_gpu(mask)
            D, H, W = mask.shape
            if min(D, H, W) < 1 or D * H * W >= 2 ** 31:
                raise ValueError(f"mesh_remove_vertices: mask volume {tuple(mask.shape)} is empty or has 2^31 voxels or more")
            mask = (mask != 0).to(torch.uint8).contiguous()
        if V == 0:
            return meshes if isinstance(meshes, Meshes) else Meshes([meshes[0]], [meshes[1]])
        vkeep = torch.empty(V, dtype=torch.uint8, device=dev)
        fkeep = torch.empty(F, dtype=torch.uint8, device=dev)
        used = torch.zeros(V, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("fsg_mesh_keep_flags_u8", _p(pk.verts), V, _p(pk.voff_t), B, _p(keep), _p(boxes), _p(mask), D, H, W, *sp, _p(vkeep),
                      _stream())
            if F:                                                            # (an empty tensor has no address to hand over)
                _lib.call("fsg_mesh_face_flags_u8", _p(pk.faces), V, F, _p(vkeep), _p(face_keep), _p(fkeep), _p(used), _stream())
            vflag = used if drop_unreferenced else vkeep
            vnew = torch.cumsum(vflag, 0, dtype=torch.int64)
            vnew = torch.cat([vnew.new_zeros(1), vnew])                      # exclusive, with the total behind
            fnew = torch.cumsum(fkeep, 0, dtype=torch.int64)
            fnew = torch.cat([fnew.new_zeros(1), fnew])
            host = torch.cat([vnew[pk.voff_t.long()], fnew[pk.foff_t]]).tolist()   # the readback: the sizes depend on the data
            vo, fo = host[:B + 1], host[B + 1:]
            verts = torch.empty(vo[-1], 3, dtype=torch.float32, device=dev)
            normals = None if pk.normals is None else torch.empty(vo[-1], 3, dtype=torch.float32, device=dev)
            faces = torch.empty(fo[-1], 3, dtype=torch.int64, device=dev)
            if vo[-1] > 0:
                pad = torch.zeros(3, dtype=torch.int64, device=dev)         # stands in for the face arrays of a batch without faces
                _lib.call("fsg_mesh_compact_f32", _p(pk.verts), _p(pk.normals), _p(pk.faces if F else pad.int()), V, F, _p(pk.voff_t),
                          B, _p(vflag), _p(vnew), _p(fkeep if F else pad.to(torch.uint8)), _p(fnew), _p(verts), _p(normals),
                          _p(faces if fo[-1] else pad), _stream())
        cut = lambda t, o: [t[o[m]:o[m + 1]] for m in range(B)]             # noqa: E731
        return Meshes(cut(verts, vo), cut(faces, fo), None if normals is None else cut(normals, vo))


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
    with torch.cuda.device(x.device):
        _lib.call("fsg_reg_smooth3_f32", _p(x), B, C, S0, S1, S2, _p(out), _stream())
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
    with torch.cuda.device(disp.device):
        _lib.call("fsg_reg_objective_f16", _p(disp), _p(feat_fix), _p(feat_mov), B, C, feat_fix.shape[4], S0, S1, S2,
                  float(lambda_weight), float(cost_scale), _p(grad), _p(loss), _p(ws), ws.numel(), _stream())


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


# ------------------------------------------------------------------ voxel CNN inference (csrc/seg_cnn.hip)
MBCONV_MAX_CIN, MBCONV_MAX_CMID, MBCONV_MAX_COUT = _lib.MBCONV_MAX_CIN, _lib.MBCONV_MAX_CMID, _lib.MBCONV_MAX_COUT


def _ndhwc(x):
    """(B, C, D, H, W) -> the (B, D, H, W, C) buffer behind it, without a copy when x is in channels-last memory"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def mbconv3d(x, w1, s1, b1, wd, s2, b2, w3, s3, b3, stride=1, residual=False, first=False):
    """One eval-mode inverted-residual block of models/mobilenet.py in one launch (fsg_mbconv3d_fwd_f32); inference only, no
    autograd.  x (B, Cin, D, H, W) fp32 on the GPU, read in `torch.channels_last_3d` memory (any other layout is copied into it)
    -> (B, Cout, Do, Ho, Wo) in the same memory format.  w1 (Cmid, Cin[, 1, 1, 1]), or with `first` the dense 3x3x3 stride-2
    padding-1 kernel (Cmid, 1, 3, 3, 3); wd (Cmid, 1, 3, 3, 3) the depthwise kernel of `stride` 1 | 2; w3 (Cout, Cmid[, 1, 1, 1]);
    (s, b) the three folded BatchNorms, ReLU6 after the first two; `residual` adds x.  Cin, Cout <= 64, Cmid a multiple of 16,
    <= 384."""
    if x.dim() != 5:
        raise ValueError(f"mbconv3d: x must be (B, Cin, D, H, W), got {tuple(x.shape)}")
    B, Cin, D, H, W = x.shape
    Cmid, Cout = wd.shape[0], w3.shape[0]
    if not (1 <= Cin <= MBCONV_MAX_CIN and 1 <= Cout <= MBCONV_MAX_COUT and 16 <= Cmid <= MBCONV_MAX_CMID and Cmid % 16 == 0):
        raise ValueError(f"mbconv3d: channels {Cin} -> {Cmid} -> {Cout} outside the kernel's limits (Cin, Cout <= 64; Cmid a "
                         f"multiple of 16, <= 384)")
    if stride not in (1, 2):
        raise ValueError(f"mbconv3d: stride must be 1 or 2, got {stride}")
    if first and Cin != 1:
        raise ValueError(f"mbconv3d: the dense first layer takes one input channel, got {Cin}")
    if residual and (first or stride != 1 or Cin != Cout):
        raise ValueError("mbconv3d: the residual add needs stride 1, Cin == Cout and the 1x1x1 expand stage")
    k1 = 27 if first else Cin
    if w1.numel() != Cmid * k1 or wd.numel() != Cmid * 27 or w3.numel() != Cout * Cmid:
        raise ValueError(f"mbconv3d: weights {tuple(w1.shape)}, {tuple(wd.shape)}, {tuple(w3.shape)} do not fit "
                         f"{Cin} -> {Cmid} -> {Cout}")
    for t, n in ((s1, Cmid), (b1, Cmid), (s2, Cmid), (b2, Cmid), (s3, Cout), (b3, Cout)):
        if t.numel() != n:
            raise ValueError("mbconv3d: a scale / shift vector does not have one entry per channel")
    _need_gpu(x, w1, s1, b1, wd, s2, b2, w3, s3, b3)
    dm = [(n - 1) // 2 + 1 for n in (D, H, W)] if first else [D, H, W]
    do = [(n - 1) // stride + 1 for n in dm]
    xc = _ndhwc(x.detach().to(torch.float32))
    y = torch.empty((B, *do, Cout), dtype=torch.float32, device=x.device)
    w1, wd, w3, s1, b1, s2, b2, s3, b3 = (_f32c(t) for t in (w1, wd, w3, s1, b1, s2, b2, s3, b3))
    with torch.cuda.device(x.device):
        _lib.call("fsg_mbconv3d_fwd_f32", _p(xc), _p(w1), _p(s1), _p(b1), _p(wd), _p(s2), _p(b2), _p(w3), _p(s3), _p(b3), B, Cin,
                  Cmid, Cout, D, H, W, int(stride), int(bool(first)), int(bool(residual)), _p(y), _stream())
    return y.permute(0, 4, 1, 2, 3)


def patch_accumulate(logits, starts, patch_size, out_sum, out_weight, weight_map=None):
    """The tail of the reference's patch loop (models/seg_cnn.py:48-59) for P patches (fsg_patch_accumulate_f32): logits
    (P, K, pd/2, ph/2, pw/2) the head's half-resolution output, starts a list of P (item, z, y, x), patch_size (pd, ph, pw),
    weight_map (pd, ph, pw) | None (weight 1).  x2 trilinear up-sampling, softmax over K, times the weight, cropped to the
    volume and added IN PLACE into out_sum (B, K, D, H, W) and out_weight (B, 1, D, H, W), patch after patch in the order given."""
    pd, ph, pw = (int(p) for p in patch_size)
    if logits.dim() != 5 or tuple(logits.shape[2:]) != (pd // 2, ph // 2, pw // 2) or pd % 2 or ph % 2 or pw % 2:
        raise ValueError(f"patch_accumulate: logits {tuple(logits.shape)} are not the half-resolution output of patches {patch_size}")
    P, K = logits.shape[:2]
    B, K2, D, H, W = out_sum.shape
    if K2 != K or tuple(out_weight.shape) != (B, 1, D, H, W) or len(starts) != P:
        raise ValueError("patch_accumulate: out_sum (B, K, D, H, W), out_weight (B, 1, D, H, W) and one start per patch expected")
    for t in (out_sum, out_weight):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("patch_accumulate: out_sum and out_weight must be contiguous fp32 (they are updated in place)")
    if weight_map is not None and tuple(weight_map.shape[-3:]) != (pd, ph, pw):
        raise ValueError(f"patch_accumulate: weight_map {tuple(weight_map.shape)} does not cover a patch {patch_size}")
    _need_gpu(logits, out_sum, out_weight, weight_map)
    host = (ctypes.c_int * (4 * P))(*[int(v) for s in starts for v in s])
    lg = _f32c(logits)
    wm = _f32c(weight_map) if weight_map is not None else None
    with torch.cuda.device(logits.device):
        _lib.call("fsg_patch_accumulate_f32", _p(lg), P, K, pd, ph, pw, host, _p(wm), _p(out_sum), _p(out_weight), B, D, H, W,
                  _stream())


def patch_finalize(out_sum, out_weight):
    """softmax over K of out_sum / out_weight (models/seg_cnn.py:61-62; fsg_patch_finalize_f32) -> a new (B, K, D, H, W) tensor"""
    _need_gpu(out_sum, out_weight)
    B, K, D, H, W = out_sum.shape
    if tuple(out_weight.shape) != (B, 1, D, H, W):
        raise ValueError("patch_finalize: out_weight must be (B, 1, D, H, W)")
    s, w = _f32c(out_sum), _f32c(out_weight)
    out = torch.empty_like(s)
    with torch.cuda.device(s.device):
        _lib.call("fsg_patch_finalize_f32", _p(s), _p(w), B, K, D, H, W, _p(out), _stream())
    return out
