"""OPTICS clustering of a pooled cloud: the 'cluster' mode of the reference's data_set_correspondences
(shape_model/generate_corresponding_points.py:50-62), which calls sklearn.cluster.OPTICS on the CPU.

The reachability ordering -- the O(n^2) part -- runs on the GPU (`functional.optics`, csrc/optics.hip).  What follows it is here
and runs on the host in numpy, because it is one sequential O(n) walk over the reachability plot:

`optics_xi_labels`  the xi extraction of Ankerst, Breunig, Kriegel, Sander, "OPTICS: Ordering Points To Identify the Clustering
  Structure" (SIGMOD 1999), section 4.3: xi-steep points, maximal steep areas, the `mib` (maximum in between) filter of the open
  steep-down areas, and cluster conditions 3b and 4 for every pair of a steep-down and a steep-up area; then the predecessor
  correction of Schubert and Gertz, "Improving the Cluster Structure Extracted from OPTICS Plots" (LWDA 2018): the end of a
  candidate is pulled in until the predecessor of its last point lies inside it.  The conventions are sklearn's
  (`cluster_optics_xi`), so that the labels equal its labels: an inf is appended to the plot; a steep area may hold at most
  min_samples consecutive points that are not steep; min_cluster_size defaults to min_samples; labels are handed out
  smallest-first (the candidates in the order found, inner before outer) and a candidate that overlaps a labelled point is
  dropped, so the leaves of the hierarchy get the labels.
`optics_cluster_centroids`  ordering on the GPU, square roots and labels on the host (so no label depends on a device square
  root), the mean of every cluster in fp64 with the points added in ascending order: the same bits on every run."""
import numpy as np
import torch

from .. import functional as F_hip


def _steep_area_end(steep, against, start, min_samples):
    """the last steep point of the maximal steep area that starts at `start`: it goes on over points that are not steep as
    long as none of them runs against the area's direction and no more than min_samples of them follow one another"""
    end, flat = start, 0
    for i in range(start, len(steep)):
        if steep[i]:
            end, flat = i, 0
        elif against[i]:
            break
        else:
            flat += 1
            if flat > min_samples:
                break
    return end


def _pull_in_end(plot, pred_plot, position, start, end):
    """Schubert & Gertz: a candidate [start, end] stands if it begins above its end, or once the predecessor of its last point
    is one of the points before that; else the last point leaves.  -> (start, end) or None"""
    while start < end:
        if plot[start] > plot[end]:
            return start, end
        p = pred_plot[end]
        if p >= 0 and start <= position[p] < end:
            return start, end
        end -= 1
    return None


def _xi_candidates(plot, pred_plot, ordering, xi, min_samples, min_cluster_size, predecessor_correction):
    """plot, pred_plot: reachability and predecessor in processing order -> [(start, end)] inclusive, inner clusters first"""
    n = len(plot)
    r = np.append(plot, np.inf)
    keep = 1.0 - xi
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = r[:-1] / r[1:]            # inf / inf = nan: such a point is neither steep nor up nor down
        steep_up, steep_down = ratio <= keep, ratio >= 1.0 / keep
        down, up = ratio > 1.0, ratio < 1.0
    position = np.empty(n, np.int64)
    position[ordering] = np.arange(n)
    open_down = []                         # steep-down areas a later steep-up area may still close: [start, end, mib]
    found = []
    at, mib = 0, 0.0                       # first point not yet inside an area; largest reachability since the last area

    def close_areas_above(level):
        """the mib filter: past an inf nothing stays open; an area stays open while the level in between is below its start
        by the factor 1 - xi, and remembers the highest level seen since it ended"""
        if np.isinf(level):
            return []
        still = [a for a in open_down if level <= r[a[0]] * keep]
        for a in still:
            a[2] = max(a[2], level)
        return still

    for i in np.flatnonzero(steep_up | steep_down).tolist():
        if i < at:
            continue
        mib = max(mib, float(r[at:i + 1].max()))
        open_down = close_areas_above(mib)
        if steep_down[i]:
            end = _steep_area_end(steep_down, up, i, min_samples)
            open_down.append([i, end, 0.0])
        else:
            end = _steep_area_end(steep_up, down, i, min_samples)
            after = r[end + 1]             # the reachability that follows the steep-up area
            here = []
            for d_start, d_end, d_mib in open_down:
                if after * keep < d_mib:   # condition sc2*: something in between is as high as the borders
                    continue
                s, e = d_start, end
                top = r[d_start]
                if top * keep >= after:    # condition 4: the down area starts higher -> begin where it has come down to `after`
                    while r[s + 1] > after and s < d_end:
                        s += 1
                elif after * keep >= top:  # the up area ends higher -> stop where it has climbed to the start level
                    while r[e - 1] > top and e > i:
                        e -= 1
                if predecessor_correction:
                    fixed = _pull_in_end(r, pred_plot, position, s, e)
                    if fixed is None:
                        continue
                    s, e = fixed
                if e - s + 1 < min_cluster_size or s > d_end or e < i:   # conditions 3a, 1 and 2
                    continue
                here.append((s, e))
            found.extend(reversed(here))   # the latest down area gives the innermost cluster
        at = end + 1
        mib = float(r[at])
    return found


def optics_xi_labels(reachability, predecessor, ordering, min_samples, min_cluster_size=None, xi=0.05,
                     predecessor_correction=True):
    """Cluster labels from an OPTICS graph by the xi method: reachability (n,) (distances, not squares; inf where undefined),
    predecessor (n,) (-1 where none) and ordering (n,), all indexed as `functional.optics` returns them -> labels (n,) int64,
    -1 for noise.  numpy arrays or tensors (copied to the host).  min_cluster_size is a count >= 2 or a fraction of n in
    (0, 1]; None means min_samples.  Equal to sklearn.cluster.cluster_optics_xi label for label."""
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)   # noqa: E731
    reach, pred, order = host(reachability).astype(np.float64), host(predecessor).astype(np.int64), host(ordering).astype(np.int64)
    n = len(order)
    if reach.shape != (n,) or pred.shape != (n,) or order.ndim != 1:
        raise ValueError(f"optics_xi_labels: reachability {reach.shape}, predecessor {pred.shape} and ordering {order.shape} must "
                         f"be vectors of one length")
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or not 2 <= min_samples <= max(n, 2):
        raise ValueError(f"optics_xi_labels: min_samples must be an integer in 2 .. n={n}, got {min_samples!r}")
    if not 0.0 <= xi <= 1.0:
        raise ValueError(f"optics_xi_labels: xi must be in [0, 1], got {xi!r}")
    if min_cluster_size is None:
        min_cluster_size = int(min_samples)
    elif isinstance(min_cluster_size, (int, np.integer)) and not isinstance(min_cluster_size, bool):
        if not 2 <= min_cluster_size <= max(n, 2):
            raise ValueError(f"optics_xi_labels: min_cluster_size must be in 2 .. n={n}, got {min_cluster_size!r}")
    elif isinstance(min_cluster_size, float) and 0.0 < min_cluster_size <= 1.0:
        min_cluster_size = max(2, int(min_cluster_size * n))
    else:
        raise ValueError(f"optics_xi_labels: min_cluster_size must be an integer >= 2 or a fraction in (0, 1], got "
                         f"{min_cluster_size!r}")
    if n == 0 or sorted(order.tolist()) != list(range(n)):
        raise ValueError("optics_xi_labels: ordering must be a permutation of 0 .. n-1")
    found = _xi_candidates(reach[order], pred[order], order, float(xi), int(min_samples), int(min_cluster_size),
                           bool(predecessor_correction))
    plot_labels = np.full(n, -1, np.int64)
    label = 0
    for s, e in found:
        if (plot_labels[s:e + 1] == -1).all():
            plot_labels[s:e + 1] = label
            label += 1
    labels = np.empty(n, np.int64)
    labels[order] = plot_labels
    return labels


def cluster_means(points, labels):
    """points (n,3), labels (n,) -> (C,3) fp64: the mean of every cluster 0 .. C-1, its points added in ascending order"""
    pts = np.asarray(points, np.float64)
    C = int(labels.max()) + 1 if len(labels) else 0
    out = np.empty((max(C, 0), 3), np.float64)
    for c in range(C):
        member = pts[labels == c]
        out[c] = np.cumsum(member, 0)[-1] / np.float64(len(member))   # cumsum adds strictly one after the other
    return out


def optics_cluster_centroids(pool, min_samples, max_eps=float("inf"), xi=0.05):
    """pool (n,3) GPU tensor -> (centroids (C,3) fp64 on the pool's device, labels (n,) int64 there): OPTICS ordering on the
    GPU, xi labels and the fp64 cluster means on the host.  C may be 0."""
    if not torch.is_tensor(pool):
        raise TypeError(f"optics_cluster_centroids: pool must be a torch tensor on the GPU, got {type(pool).__name__}")
    if pool.dim() != 2:
        raise ValueError(f"optics_cluster_centroids: expected a pool (n,3), got {tuple(pool.shape)}")
    ordering, _, reach2, pred = F_hip.optics(pool, min_samples, max_eps, return_squared=True)
    labels = optics_xi_labels(np.sqrt(reach2.cpu().numpy()), pred.cpu().numpy(), ordering.cpu().numpy(), min_samples, xi=xi)
    centroids = cluster_means(pool.detach().float().cpu().numpy(), labels)
    return torch.from_numpy(centroids).to(pool.device), torch.from_numpy(labels).to(pool.device)
