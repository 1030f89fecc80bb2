"""Point cloud <-> dense grid, the spectral PSR solve (csrc/grid_points.hip); marching cubes (csrc/marching_cubes.hip)."""
import torch

from .. import _lib
from .._launch import _amp_bwd, _amp_fwd, _f32c, _need_gpu, _p, _stream, launch


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
        launch(grid.device, "fsg_grid_sample_f32", _p(grid), _p(coords), _p(weights), B, C, N, D, H, W, m, _p(sampled), _p(gc))
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
    launch(x.device, "fsg_psr_spectral_f32", _p(x), B, R0, R1, R2, float(sig), int(adjoint), _p(out))
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
