"""Random-walker segmentation with the reference's names (data_processing/random_walk.py:15-116), tensors in, tensors out.
The graph Laplacian is never built on the hot path: `compute_laplace_matrix` returns a small object holding the image and
the weight mode, and `random_walk` hands both to the matrix-free solver (csrc/random_walk.hip).  Instead of the reference's
pyamg Ruge-Stueben hierarchy the systems run Jacobi-preconditioned conjugate gradients to the same relative tolerance (1e-3);
the two iterates agree to that tolerance, not bit for bit."""
import torch

from .. import functional as F_hip

SIGMA = 8          # random_walk.py:24
LAMBDA = 1         # :25
EPSILON = .00001   # :73


class ImageGraphLaplacian:
    """What compute_laplace_matrix returns here: the image and the edge-weight mode, which define the operator."""

    def __init__(self, im, edge_weights):
        if edge_weights not in ("binary", "intensity"):
            raise ValueError(f'No edge weights named "{edge_weights}" known.')
        self.im = im
        self.edge_weights = edge_weights

    @property
    def shape(self):
        n = self.im.numel()
        return torch.Size([n, n])

    def to_sparse(self):
        """the reference's matrix (random_walk.py:26-77) as a coalesced fp32 COO tensor on the device of `im`: for tests and
        small inputs only (it holds seven entries per voxel)"""
        im = self.im
        n = im.numel()
        ind = torch.arange(n, device=im.device).view(*im.size())
        flat = im.reshape(-1)
        A = None
        for dim in range(im.dim()):
            i_from = ind.narrow(dim, 0, im.shape[dim] - 1).reshape(-1)
            i_to = ind.narrow(dim, 1, im.shape[dim] - 1).reshape(-1)
            if self.edge_weights == "intensity":
                val = torch.exp(-(flat[i_from] - flat[i_to]).pow(2) / (2 * SIGMA ** 2))
            else:
                val = torch.where(flat[i_from] == flat[i_to], 1., 0.01)
            a = torch.sparse_coo_tensor(torch.stack((i_from, i_to)), val.float(), (n, n))
            a = a + a.t()
            A = a if A is None else A + a
        deg = torch.sparse.sum(A, 0).to_dense()
        diag = torch.sparse_coo_tensor(torch.stack((ind.view(-1), ind.view(-1))), EPSILON + LAMBDA * deg, (n, n))
        return (diag + A * (-LAMBDA)).coalesce()


def compute_laplace_matrix(im: torch.Tensor, edge_weights: str, graph_mask: torch.Tensor = None) -> ImageGraphLaplacian:
    """random_walk.py:15-77.  `graph_mask` is not supported: in the reference only a toy example passes it, and its edge
    filter tests one endpoint twice (:45); pass the mask to `random_walk` instead, as fill_lobes does."""
    if graph_mask is not None:
        raise NotImplementedError("compute_laplace_matrix: graph_mask is not supported; pass the mask to random_walk")
    return ImageGraphLaplacian(im, edge_weights)


def random_walk(L: ImageGraphLaplacian, labels: torch.Tensor, graph_mask: torch.Tensor = None, **solver) -> torch.Tensor:
    """random_walk.py:80-116: labels in 0..N (0 = unseeded), graph_mask the voxels that take part -> probabilities
    (*labels.shape, N) fp32: one-hot at seeds, 0 outside the mask.  Keyword arguments go to functional.random_walk_solve."""
    if not isinstance(L, ImageGraphLaplacian):
        raise TypeError("random_walk expects the ImageGraphLaplacian that compute_laplace_matrix returns")
    if labels.dim() not in (2, 3):
        raise ValueError(f"random_walk: labels (H, W) or (D, H, W), got {tuple(labels.shape)}")
    return F_hip.random_walk_solve(L.im, labels, graph_mask, L.edge_weights, **solver)
