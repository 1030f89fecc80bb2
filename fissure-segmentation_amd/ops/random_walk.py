"""Random-walker solve and filling, lobes to fissures (csrc/random_walk.hip)."""
import torch

from .. import _lib
from .._launch import _f32c, _need_gpu, _p, _stream, launch


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
        launch(lc.device, "fsg_lobes_to_fissures_u8", _p(lc), B, D, H, W, hi, _p(out))
    return out
