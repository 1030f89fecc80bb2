"""Benchmark of the mesh -> label map kernels (csrc/voxelize.hip) beside the route the package had before them.

    python tools/bench_voxelize.py [--quick]

Shapes: 128^3 and 256 x 256 x 320 voxels, spacing 1 mm, three noisy tilted sheets of 51 x 51 vertices (5000 faces each) across the
volume (tests/voxelize_oracle.sheet), threshold 1.0.  Timed with HIP events around whole calls of the public functions (so
packing, allocation and the memset are inside), median and minimum of `iters` calls after a warm-up, the candidates
alternating:

* functional.mesh_labelmap_dist, functional.mesh_labelmap_cover;
* the brute-force route: functional.point_mesh_distance from ALL voxel centres to each mesh, then torch's argmin and
  threshold -- voxels x faces pair evaluations;
* the floor of a mesh_labelmap_dist call: one face outside the volume, i.e. key-volume memset + decode pass, and torch's
  fill of a key volume alone;
* both kernels on ONE face whose bounding box is the whole volume (one wave walks all of it).

Counted on the host in fp64 (not timed): the voxels the band kernel visits (boxes grown by the threshold) and the atomics it
issues (visited voxels within the threshold of their face); the cells the coverage kernel visits.  The two routes' label
maps are compared voxel by voxel.  One JSON line per shape on stdout."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fissure_segmentation_amd as fsg  # noqa: E402
import metrics_oracle as mo  # noqa: E402
import voxelize_oracle as vo  # noqa: E402

F = fsg.functional
dev = torch.device("cuda:0")
THR = 1.0


def timed(fns, iters, warm=3):
    """{name: (median us, min us)} of several candidates, alternating"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3)
    return {k: (round(statistics.median(v), 1), round(min(v), 1)) for k, v in ts.items()}


def host_counts(meshes, shape, spacing, thr):
    """(voxels visited by the band kernel, atomics it issues, cells visited by the coverage kernel), fp64 on the host"""
    s, n = np.asarray(spacing), np.asarray(shape)
    visited = atomics = cells = 0
    for verts, faces in meshes:
        tri = verts[faces]
        lo, hi = tri.min(1), tri.max(1)
        first = np.maximum(np.ceil((lo - thr) / s), 0).astype(np.int64)
        last = np.minimum(np.floor((hi + thr) / s), n - 1).astype(np.int64)
        cfirst = np.maximum(np.floor(lo / s), 0).astype(np.int64)
        clast = np.minimum(np.floor(hi / s), n - 1).astype(np.int64)
        cells += int(np.prod(np.maximum(clast - cfirst + 1, 0), 1).sum())
        for t, a, b in zip(tri, first, last):
            if (a > b).any():
                continue
            q = np.stack(np.meshgrid(*[np.arange(x, y + 1) for x, y in zip(a, b)], indexing="ij"), -1).reshape(-1, 3) * s
            t = torch.from_numpy(t)
            d2 = mo.tri_dist2(torch.from_numpy(q), t[0], t[1], t[2])
            visited += len(q)
            atomics += int((d2 <= thr * thr).sum())
    return visited, atomics, cells


def main():
    quick = "--quick" in sys.argv
    shapes = [(32, 32, 40)] if quick else [(128, 128, 128), (256, 256, 320)]
    for shape in shapes:
        spacing = (1.0, 1.0, 1.0)
        n_side = 11 if quick else 51
        meshes = [vo.sheet(seed, tilt, shape, spacing, n=n_side) for seed, tilt in vo.SHEETS]
        verts = [torch.from_numpy(v).to(dev, torch.float32) for v, _ in meshes]
        faces = [torch.from_numpy(f).to(dev, torch.int32) for _, f in meshes]
        nvox, nfaces = int(np.prod(shape)), sum(len(f) for f in faces)
        centres = torch.from_numpy(vo.voxel_centres(shape, spacing)).to(dev, torch.float32)[None]
        far_v = torch.tensor([[-9., -9, -9], [-8, -9, -9], [-9, -8, -9]], device=dev)
        far_f = torch.tensor([[0, 1, 2]], device=dev, dtype=torch.int32)
        keys = torch.empty(shape, dtype=torch.int64, device=dev)
        e = torch.tensor(vo.extent(shape, spacing))
        huge_v = (torch.stack([e * torch.tensor([-1., -1, 0.4]), e * torch.tensor([3., -1, 0.5]), e * torch.tensor([-1., 3, 0.6])]) + 0.0137
                  ).to(dev, torch.float32)                                          # one face whose box is the whole volume

        def brute():
            d = torch.stack([F.point_mesh_distance(centres, v[None], f, validate=False)[0] for v, f in zip(verts, faces)])
            best = d.argmin(0)
            return torch.where(d.gather(0, best[None])[0] <= THR, best + 1, 0).reshape(shape)

        fns = {"dist": lambda: F.mesh_labelmap_dist(verts, faces, shape, spacing, THR, validate=False),
               "cover": lambda: F.mesh_labelmap_cover(verts, faces, shape, spacing, validate=False),
               "dist_floor": lambda: F.mesh_labelmap_dist([far_v], [far_f], shape, spacing, THR, validate=False),
               "key_fill": lambda: keys.fill_(-1),
               "dist_whole_volume_face": lambda: F.mesh_labelmap_dist([huge_v], [far_f], shape, spacing, THR, validate=False),
               "cover_whole_volume_face": lambda: F.mesh_labelmap_cover([huge_v], [far_f], shape, spacing, validate=False)}
        res = timed(fns, iters=5 if quick else 30)
        res.update(timed({"brute_force": brute}, iters=2 if quick else 5, warm=1))
        got, want = fns["dist"](), brute()
        visited, atomics, cells = host_counts(meshes, shape, spacing, THR)
        print(json.dumps({"device": torch.cuda.get_device_name(0), "shape": shape, "voxels": nvox, "faces": nfaces, "threshold": THR,
                          "us_median_min": res, "speedup_dist_vs_brute_force": round(res["brute_force"][0] / res["dist"][0], 1),
                          "pairs_brute_force": nvox * nfaces, "pairs_dist": visited, "atomics_dist": atomics, "cells_cover": cells,
                          "labelled_dist": int((got != 0).sum()), "labelled_cover": int((fns["cover"]() != 0).sum()),
                          "voxels_differing_from_brute_force": int((got != want).sum())}), flush=True)


if __name__ == "__main__":
    main()
