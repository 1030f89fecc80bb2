"""DSEG-AE (dseg_ae_regularization.py of the reference): segment a cloud with `DGCNNSeg`, take every object's points, optionally
pad them with jittered copies, pick `n_points_ae` of them by farthest point sampling and let the point-cloud auto-encoder
(`DGCNNFoldingNet`) fold a regular mesh onto them.

Same names, arguments and return structure as the reference for one cloud (`segment`, `reconstruct`, `forward`,
`random_extend_points`, `farthest_point_sampling`); `reconstruct_packed` is the batched form underneath, which serves every
(item, object) group of any batch with one partition (csrc/dseg_ae.hip: fsg_label_partition), one extension launch
(fsg_segment_jitter_extend_f32), one sampling launch (fsg_fps_start_f32) and one auto-encoder forward per distinct input size.

Ours, not the reference's:
  * nearest-neighbour distances are the direct form (x - y)^2 (`functional.knn_segment`), which never gives the NaN that the
    reference's xx - 2 xy + yy form gives for the square root of a slightly negative distance;
  * the jitter statistics are per item (the reference pools them over the tensor and is only ever called with B = 1);
  * sampling ties go to the lowest index (the reference's argmax takes the first maximum, which is the same rule);
  * any batch size.
Not mirrored: file and data set handling, CSV, plots, the k-means / PCA of the hidden codes, `speed_test` and the command line
(:141-212, :249-468; `reconstruction_metrics` stands for :213-247).
"""
import torch

from . import functional as F_hip
from .metrics import assd, pseudo_symmetric_point_to_mesh_distance
from .models.dgcnn import DGCNNSeg
from .models.folding_net import DGCNNFoldingNet
from .models.modelio import LoadableModel, store_config_args
from .utils.general_utils import farthest_point_sampling  # noqa: F401  (the reference defines it here, :30-43)

ACCUMULATE_RUNS = 10   # :92


def _extend_draws(n_points, n_pad, batch, device):
    """the reference's three draws in the reference's order (:128, :131, :133): source rows on the CPU generator (one list
    for the whole batch), directions and magnitudes on the device"""
    src = torch.randint(n_points, (n_pad,))
    direction = torch.randn(batch, n_pad, 3, device=device)
    z = torch.randn(batch, n_pad, 1, device=device)
    return src, direction, z


def random_extend_points(points, desired_n_points, draws=None):
    """points (B, n, 3) -> (B, max(n, desired_n_points), 3): the cloud, then randomly chosen points of it moved in a random
    direction by a random length with the mean and standard deviation of the cloud's nearest-neighbour distances (:115-138).
    One launch for the batch, one segment per item; the statistics are per item.  `draws` = (src (n_pad,) int, direction
    (B, n_pad, 3), z (B, n_pad, 1)) replaces the random numbers; without it they are drawn as the reference draws them."""
    B, n_points = points.shape[0], points.shape[1]
    n_pad = desired_n_points - n_points
    if n_pad <= 0:
        return points
    src, direction, z = _extend_draws(n_points, n_pad, B, points.device) if draws is None else draws
    out, _, _ = F_hip.segment_jitter_extend(
        points.reshape(B * n_points, 3), [n_points * (b + 1) for b in range(B)], desired_n_points,
        src.to(points.device).repeat(B), direction.reshape(B * n_pad, 3), z.reshape(B * n_pad))
    return out.view(B, desired_n_points, 3).to(points.dtype)


class RegularizedSegDGCNN(LoadableModel):
    """:46-112.  `seg_model` and `ae` are checkpoint paths; the sub-modules carry those names, so a reference checkpoint's keys
    load."""

    @store_config_args
    def __init__(self, seg_model, ae, n_points_seg, n_points_ae, sample_mode='farthest', random_extend=False):
        super().__init__()
        self.seg_model = DGCNNSeg.load(seg_model, 'cpu')
        self.ae = DGCNNFoldingNet.load(ae, 'cpu')
        self.n_points_seg = n_points_seg
        self.n_points_ae = n_points_ae
        self.sample_mode = sample_mode
        self.random_extend = random_extend

    @torch.no_grad()
    def segment(self, x):
        return self.seg_model.predict_full_pointcloud(x, self.n_points_seg).argmax(1)

    def _check_mode(self, return_hidden):
        if self.sample_mode == 'accumulate':
            if return_hidden:
                raise NotImplementedError('Hidden output not implemented for accumulate sampling.')
        elif self.sample_mode != 'farthest':
            raise NotImplementedError(f'Sampling mode {self.sample_mode} not implemented.')

    def _ae_vertices(self, pts, return_hidden):
        """pts (G, s, 3) -> vertices (G, m, 3) and the hidden codes (G, 1, E) or None: one auto-encoder forward"""
        out = self.ae(pts.transpose(1, 2).contiguous(), return_hidden=return_hidden)
        out, hidden = out if return_hidden else (out, None)
        verts = out.verts_padded() if hasattr(out, "verts_padded") else out.transpose(1, 2)
        return verts, hidden

    @torch.no_grad()
    def reconstruct_packed(self, x, seg, return_hidden=False):
        """x (B, C, N) with the coordinates in channels 0..2, seg (B, N) labels -> a dict over the G = B (num_classes - 1)
        groups, in (item, object) order:
          'vertices' (G, m, 3): the auto-encoder's output (zeros where not valid);
          'group' (G, 2) int64 on the CPU: item and object label of every group;
          'valid' (G) bool on the CPU: the object has at least `ae.encoder.k` points;
          'points' (n_s, 3) with 'points_offset' (G) on the CPU (segment ends): the auto-encoder's input of a valid group in
              'farthest' mode, the object's (extended) points in 'accumulate' mode, the raw points of a group that is not valid;
          'index' (n_s) int64: the row of every point of 'points' in the extended object (rows >= the object's length are
              jittered copies), 'source' (n) int32 with 'source_offset': the index inside its item of every original point;
          'hidden' (G, 1, E) or None.
        One host read per call (the group sizes, `counts`); every later size follows from them.  The random numbers are drawn
        group by group as the reference's loop draws them per object: the three of `random_extend_points`, then the
        sampling start (:37)."""
        self._check_mode(return_hidden)
        B, L, n_ae, k = x.shape[0], self.seg_model.num_classes - 1, self.n_points_ae, self.ae.encoder.k
        dev = x.device
        counts, offset, xyz, src = F_hip.label_partition(seg, x, L, first_label=1)
        lens = counts.flatten().tolist()                                   # the one host read
        G = len(lens)
        ends = torch.tensor(lens, dtype=torch.int64).cumsum(0)
        n = int(ends[-1])
        valid = [l >= k for l in lens]
        group = torch.tensor([[g // L, g % L + 1] for g in range(G)], dtype=torch.int64)
        m = self.ae.decoder.m
        out = {"group": group, "valid": torch.tensor(valid), "source": src[:n], "source_offset": ends,
               "vertices": torch.zeros(G, m, 3, device=dev), "hidden": None}
        if n == 0:
            out.update(points=xyz[:0], points_offset=ends, index=torch.zeros(0, dtype=torch.int64, device=dev))
            return out
        xyz = xyz[:n]

        # the draws, group by group in the reference's per-object order
        new_lens, starts, d_src, d_dir, d_z = list(lens), [0] * G, [], [], []
        for g in range(G):
            if not valid[g]:
                continue
            if self.random_extend and lens[g] < n_ae:
                s, d, z = _extend_draws(lens[g], n_ae - lens[g], 1, dev)
                d_src.append(s), d_dir.append(d[0]), d_z.append(z.flatten())
                new_lens[g] = n_ae
            if self.sample_mode == 'farthest' and new_lens[g] > n_ae:
                starts[g] = int(torch.randint(new_lens[g], (1,)))
        ext_ends = torch.tensor(new_lens, dtype=torch.int64).cumsum(0).tolist()
        ext_st = [e - l for e, l in zip(ext_ends, new_lens)]
        grow = [g for g in range(G) if new_lens[g] > lens[g]]
        if grow:
            # only the groups that grow go through the nearest-neighbour search and the extension launch (a group gives the
            # same bits alone and in a batch); the others keep their rows
            st = (ends - torch.tensor(lens)).tolist()
            sub = xyz if len(grow) == G else torch.cat([xyz[st[g]:st[g] + lens[g]] for g in grow])
            grown, _, _ = F_hip.segment_jitter_extend(sub, torch.tensor([lens[g] for g in grow]).cumsum(0).tolist(),
                                                      [new_lens[g] for g in grow], torch.cat(d_src).to(dev), torch.cat(d_dir),
                                                      torch.cat(d_z))
            if len(grow) == G:
                ext = grown
            else:
                parts, q = [], 0
                for g in range(G):
                    if new_lens[g] > lens[g]:
                        parts.append(grown[q:q + new_lens[g]])
                        q += new_lens[g]
                    else:
                        parts.append(xyz[st[g]:st[g] + lens[g]])
                ext = torch.cat(parts)
        else:
            ext = xyz
        ext_off = torch.tensor(ext_ends, dtype=torch.int32).to(dev)

        if self.sample_mode == 'accumulate':
            # every run of every valid group through the auto-encoder as one batch; a group's runs are averaged in run order
            vg = [g for g in range(G) if valid[g]]
            if vg:
                # (drawn group by group, run by run, like `DGCNNFoldingNet.predict_full_pointcloud` in the reference's loop)
                pick = [torch.stack([ext_st[g] + torch.randperm(new_lens[g], device=dev)[:n_ae] for _ in range(ACCUMULATE_RUNS)])
                        for g in vg]
                verts = torch.empty(len(vg), ACCUMULATE_RUNS, m, 3, device=dev)
                for size in sorted({p.shape[1] for p in pick}):     # a group shorter than n_points_ae gives runs of its own size
                    sel = [i for i, p in enumerate(pick) if p.shape[1] == size]
                    verts[sel] = self._ae_vertices(ext[torch.cat([pick[i] for i in sel])], False)[0].reshape(
                        len(sel), ACCUMULATE_RUNS, m, 3)
                acc = torch.zeros(len(vg), m, 3, device=dev)
                for r in range(ACCUMULATE_RUNS):
                    acc += verts[:, r]
                out["vertices"][vg] = acc / ACCUMULATE_RUNS
            index = torch.arange(ext.shape[0], device=dev) - torch.repeat_interleave(
                torch.tensor(ext_st, device=dev), torch.tensor(new_lens, device=dev))
            out.update(points=ext, points_offset=torch.tensor(ext_ends), index=index)
            return out

        # 'farthest': one sampling launch over the groups that are longer than n_points_ae, the others pass through in order
        m_g = [n_ae if valid[g] and new_lens[g] > n_ae else 0 for g in range(G)]
        n_fps = sum(m_g)
        if n_fps:
            fps_idx = F_hip.fps_start(ext, ext_off, torch.tensor(m_g, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev), n_fps,
                                      torch.tensor(starts, dtype=torch.int32).to(dev)).long()
        parts, q = [], 0
        for g in range(G):
            if m_g[g]:
                parts.append(fps_idx[q:q + n_ae])
                q += n_ae
            else:
                parts.append(torch.arange(ext_st[g], ext_ends[g], device=dev))
        rows = torch.cat(parts)
        s_lens = [p.shape[0] for p in parts]
        s_ends = torch.tensor(s_lens, dtype=torch.int64).cumsum(0)
        points = ext[rows]
        out.update(points=points, points_offset=s_ends,
                   index=rows - torch.repeat_interleave(torch.tensor(ext_st, device=dev), torch.tensor(s_lens, device=dev)))
        s_st = (s_ends - torch.tensor(s_lens)).tolist()
        hidden = None
        for size in sorted({s_lens[g] for g in range(G) if valid[g]}):     # one forward per distinct input size
            sel = [g for g in range(G) if valid[g] and s_lens[g] == size]
            pts = torch.stack([points[s_st[g]:s_st[g] + size] for g in sel])
            verts, h = self._ae_vertices(pts, return_hidden)
            out["vertices"][sel] = verts
            if return_hidden:
                if hidden is None:
                    hidden = torch.zeros(G, *h.shape[1:], device=dev)
                hidden[sel] = h
        out["hidden"] = hidden
        return out

    def _mesh(self, verts):
        """vertices (1, m, 3) -> what the auto-encoder returns for one cloud: `self.ae(...)` gives (1, 3, m),
        `self.ae.predict_full_pointcloud(...)` ('accumulate' mode) gives (1, m, 3); both a `mesh.Meshes` with `return_meshes`"""
        if self.ae.return_meshes and self.ae.decoder.decode_mesh:
            from .mesh import Meshes
            return Meshes(verts, self.ae.decoder.faces[:1])
        return verts if self.sample_mode == 'accumulate' else verts.transpose(1, 2)

    @torch.no_grad()
    def reconstruct(self, x, seg, return_hidden=False):
        """:62-106 for one cloud: lists over the objects 1 .. num_classes - 1 of the auto-encoder's output ((1, 3, m) in
        'farthest' mode, (1, m, 3) in 'accumulate' mode as `predict_full_pointcloud` returns it, or a `mesh.Meshes` with
        `DGCNNFoldingNet.return_meshes`), of the points it was given ((1, n, 3); every (extended) point of
        the object in 'accumulate' mode) and, with return_hidden, of the hidden codes.  An object with fewer than
        `ae.encoder.k` points gives None, its raw points and None.  A view of `reconstruct_packed`."""
        if x.shape[0] != 1:
            raise ValueError("reconstruct: one cloud at a time, as in the reference (its mask indexing needs equal object sizes "
                             "across a batch); reconstruct_packed takes any batch")
        p = self.reconstruct_packed(x, seg, return_hidden)
        ends = p["points_offset"].tolist()
        meshes, points, all_hidden = [], [], []
        for g, e in enumerate(ends):
            points.append(p["points"][(ends[g - 1] if g else 0):e].unsqueeze(0).to(x.dtype))
            ok = bool(p["valid"][g])
            meshes.append(self._mesh(p["vertices"][g:g + 1]) if ok else None)
            all_hidden.append(p["hidden"][g:g + 1] if ok and return_hidden else None)
        return (meshes, points, all_hidden) if return_hidden else (meshes, points)

    @torch.no_grad()
    def forward(self, x, return_hidden=False):
        seg = self.segment(x)
        return self.reconstruct(x, seg, return_hidden)


def _vertices(mesh):
    """the auto-encoder's output for one object -> (m, 3) vertices or points"""
    if hasattr(mesh, "verts_padded"):
        return mesh.verts_padded()[0]
    if mesh.dim() == 3:     # (1, 3, m) from a forward, (1, m, 3) from the accumulated runs
        mesh = mesh[0]
        return mesh if mesh.shape[1] == 3 and mesh.shape[0] != 3 else mesh.transpose(0, 1)
    return mesh


def reconstruction_metrics(meshes, points, inputs, target_meshes, faces=None, n_samples=10 ** 5, generator=None):
    """The per-object numbers of the reference's `test` (:213-247) for one cloud, without files or plots.  meshes, points: the
    lists `reconstruct` returns; inputs: per object the (n, 3) points to compare with (the reference: the points that carry
    the object's label); target_meshes: per object a (verts, faces) pair or an object with `.vertices` / `.triangles`.
    faces: the auto-encoder's (T, 3) triangles when its output is a mesh (`ae.decoder.faces[0]`) -- then the surface numbers
    come from `metrics.assd`; None: the output is a point cloud, measured by `pseudo_symmetric_point_to_mesh_distance`
    (n_samples, generator go there).
    -> dict of (n_objects,) CPU tensors 'chamfer', 'assd', 'sdsd', 'hd', 'hd95', NaN for a missing object (mesh None), and
    'percent_missing', a number.  Chamfer is pytorch3d's: the sum of the two mean squared nearest distances."""
    n_obj = len(meshes)
    res = {key: torch.full((n_obj,), float('nan')) for key in ('chamfer', 'assd', 'sdsd', 'hd', 'hd95')}
    for o, mesh in enumerate(meshes):
        if mesh is None:
            continue
        verts = _vertices(mesh).to(torch.float32)
        inp = inputs[o].reshape(-1, 3).to(torch.float32)
        if inp.shape[0]:
            d_xy = F_hip.chamfer_nn(verts[None].contiguous(), inp[None].contiguous())[0]
            d_yx = F_hip.chamfer_nn(inp[None].contiguous(), verts[None].contiguous())[0]
            res['chamfer'][o] = (d_xy.mean() + d_yx.mean()).cpu()
        if faces is not None:
            four = assd((verts, faces), target_meshes[o])
        else:
            four = pseudo_symmetric_point_to_mesh_distance(verts, target_meshes[o], n_samples=n_samples, generator=generator)
        for key, v in zip(('assd', 'sdsd', 'hd', 'hd95'), four):
            res[key][o] = v.detach().cpu()
    res['percent_missing'] = float(sum(m is None for m in meshes)) / max(n_obj, 1) * 100
    return res
