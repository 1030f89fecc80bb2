"""Timings of the voxel CNN (MobileNetASPP) on the GPU: HIP-event medians, every shape warmed up, fused path and torch
composition alternating in one process.  One JSON line per measurement on stdout and, with --out, appended to a file
(profiles/seg_cnn_bench.jsonl).

    python tools/bench_seg_cnn.py backbone      # fused block kernels / torch composition of the same eval backbone, 128^3, B = 1 and 4
    python tools/bench_seg_cnn.py forward       # the whole eval forward at 128^3, split into backbone / ASPP / head
    python tools/bench_seg_cnn.py patches       # predict_all_patches on 256x256x320 / the reference-shaped loop; kernels (b) alone
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT = None


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def measure(fn, iters=10, warm=3):
    """median milliseconds of fn() between two events on the current stream"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times), min(times), max(times)


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def make_net(patch=(128, 128, 128), classes=3):
    from fissure_segmentation_amd.models.seg_cnn import MobileNetASPP
    torch.manual_seed(0)
    net = MobileNetASPP(classes, patch_size=patch)
    for m in net.modules():        # running statistics and scales away from the identity, so that no stage is trivial
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    return net.cuda().eval()


def composition(folded, channels_last):
    """the same eval backbone as a torch composition: BatchNorms folded into the convolutions, clamp for ReLU6"""
    fmt = torch.channels_last_3d if channels_last else torch.contiguous_format
    blocks = []
    for (w1, s1, b1, wd, s2, b2, w3, s3, b3), kw in folded:
        v = (-1, 1, 1, 1, 1)
        blocks.append(((w1 * s1.view(v)).contiguous(memory_format=fmt), b1, (wd * s2.view(v)).contiguous(memory_format=fmt), b2,
                       (w3 * s3.view(v)).contiguous(memory_format=fmt), b3, kw))

    def run(x):
        x = x.contiguous(memory_format=fmt)
        for w1, b1, wd, b2, w3, b3, kw in blocks:
            u = F.conv3d(x, w1, b1, stride=2, padding=1) if kw["first"] else F.conv3d(x, w1, b1)
            t = F.conv3d(u.clamp_(0, 6), wd, b2, stride=kw["stride"], padding=1, groups=wd.shape[0])
            y = F.conv3d(t.clamp_(0, 6), w3, b3)
            x = y + x if kw["residual"] else y
        return x
    return run


def bench_backbone(args):
    net = make_net()
    folded = net.folded()["backbone"]
    comps = {"contiguous": composition(folded, False), "channels_last_3d": composition(folded, True)}
    for B in (1, 4):
        x = torch.randn(B, 1, 128, 128, 128, device="cuda")
        with torch.no_grad():
            fused = lambda: net.backbone.forward_fused(x, folded)[1]
            ref = comps["contiguous"](x)
            err = float((fused() - ref).abs().max() / ref.abs().max())
            t_fused = measure(fused, args.iters)
            t_comp = {k: measure(lambda f=f: f(x), args.iters) for k, f in comps.items()}
            t_fused2 = measure(fused, args.iters)          # again after the compositions: the spread between the two is the noise
            best = min(t_comp, key=lambda k: t_comp[k][0])
            emit(bench="backbone", B=B, shape=[128, 128, 128], fused_ms=round(t_fused[0], 3), fused_again_ms=round(t_fused2[0], 3),
                 fused_min_max_ms=[round(t_fused[1], 3), round(t_fused[2], 3)],
                 composition_ms={k: round(v[0], 3) for k, v in t_comp.items()}, composition_best=best,
                 ratio_composition_over_fused=round(t_comp[best][0] / t_fused[0], 3), rel_diff_to_composition=err,
                 fused_peak_extra_mib=round(peak_extra_mib(fused), 1),
                 composition_peak_extra_mib=round(peak_extra_mib(lambda: comps[best](x)), 1))
            per_block = []
            cur = x
            from fissure_segmentation_amd import functional as F_hip
            for tensors, kw in folded:
                nxt = F_hip.mbconv3d(cur, *tensors, **kw)
                per_block.append(round(measure(lambda c=cur, t=tensors, k=kw: F_hip.mbconv3d(c, *t, **k), args.iters)[0], 3))
                cur = nxt
            emit(bench="backbone_blocks", B=B, fused_block_ms=per_block)


def bench_forward(args):
    net = make_net()
    fd = net.folded()
    for B in (1, 4):
        x = torch.randn(B, 1, 128, 128, 128, device="cuda")
        with torch.no_grad():
            x1, x2 = net.backbone.forward_fused(x, fd["backbone"])

            def aspp():
                return [net.aspp.forward_folded(x2[i:i + 1], fd["aspp"]) for i in range(B)]

            ys = aspp()

            def head():
                out = []
                for i in range(B):
                    y = torch.cat([x1[i:i + 1], F.interpolate(ys[i], scale_factor=2)], dim=1)
                    y = F.relu(F.conv3d(y, *fd["head"][0]))
                    y = F.relu(F.conv3d(y, *fd["head"][1], padding=1))
                    out.append(F.conv3d(y, *fd["head"][2]))
                return F.interpolate(torch.cat(out), scale_factor=2, mode="trilinear", align_corners=False)

            emit(bench="forward", B=B, shape=[128, 128, 128], forward_ms=round(measure(lambda: net(x), args.iters)[0], 3),
                 backbone_ms=round(measure(lambda: net.backbone.forward_fused(x, fd["backbone"]), args.iters)[0], 3),
                 aspp_ms=round(measure(aspp, args.iters)[0], 3), head_and_upsampling_ms=round(measure(head, args.iters)[0], 3))


def bench_patches(args):
    from fissure_segmentation_amd import functional as F_hip
    from fissure_segmentation_amd.models import seg_cnn
    net = make_net()
    shape = (256, 256, 320)
    img = torch.randn(1, 1, *shape, device="cuda")
    patch = net.patch_size

    def reference_loop(use_gaussian=True):
        """models/seg_cnn.py:32-62 on this package's forward: one patch at a time, the tail as torch operations"""
        starts = seg_cnn.get_patch_starts(shape, 0.5, patch)
        out = torch.zeros(1, net.num_classes, *shape, device="cuda")
        norm = torch.zeros_like(out)
        g = net.gaussian_map("cuda")[None, None]
        for z in starts[0]:
            for y in starts[1]:
                for x in starts[2]:
                    region = (slice(None), slice(None), slice(z, z + patch[0]), slice(y, y + patch[1]), slice(x, x + patch[2]))
                    part = img[region]
                    before = part.shape[2:]
                    p = torch.softmax(net(seg_cnn.maybe_pad_img_patch(part, patch)), dim=1)
                    if use_gaussian:
                        p = p * g
                        norm[region] += seg_cnn.maybe_crop_after_padding(g, before)
                    else:
                        norm[region] += 1
                    out[region] += seg_cnn.maybe_crop_after_padding(p, before)
        return torch.softmax(out / norm, dim=1)

    with torch.no_grad():
        ours = lambda: net.predict_all_patches(img, patch_batch=args.patch_batch)
        diff = float((ours() - reference_loop()).abs().max())
        t_ours = measure(ours, args.patch_iters, 1)
        t_ref = measure(reference_loop, args.patch_iters, 1)
        emit(bench="predict_all_patches", shape=list(shape), patch=list(patch), patches=36, patch_batch=args.patch_batch,
             ours_ms=round(t_ours[0], 1), reference_shaped_loop_ms=round(t_ref[0], 1), ratio=round(t_ref[0] / t_ours[0], 3),
             max_abs_diff=diff, ours_peak_extra_mib=round(peak_extra_mib(ours), 1),
             loop_peak_extra_mib=round(peak_extra_mib(reference_loop), 1))
        # kernels (b) alone on one group of patches, beside their torch composition
        P = args.patch_batch
        logits = torch.randn(P, net.num_classes, *(p // 2 for p in patch), device="cuda")
        entries = [(0, 0, 0, 64 * i) for i in range(P)]
        out_sum, out_w = torch.zeros(1, net.num_classes, *shape, device="cuda"), torch.zeros(1, 1, *shape, device="cuda")
        g = net.gaussian_map("cuda")
        norm = torch.zeros_like(out_sum)

        def torch_tail():
            for lg, (_, z, y, x) in zip(logits, entries):
                p = torch.softmax(F.interpolate(lg[None], scale_factor=2, mode="trilinear", align_corners=False), dim=1) * g
                region = (slice(None), slice(None), slice(z, z + patch[0]), slice(y, y + patch[1]), slice(x, x + patch[2]))
                norm[region] += g
                out_sum[region] += p

        t_k = measure(lambda: F_hip.patch_accumulate(logits, entries, patch, out_sum, out_w, g), args.iters)
        t_t = measure(torch_tail, args.iters)
        out_w.clamp_(min=1e-3)
        norm.clamp_(min=1e-3)
        t_fk = measure(lambda: F_hip.patch_finalize(out_sum, out_w), args.iters)
        t_ft = measure(lambda: torch.softmax(out_sum / norm, dim=1), args.iters)
        emit(bench="patch_kernels", patches=P, accumulate_ms=round(t_k[0], 3), accumulate_torch_ms=round(t_t[0], 3),
             finalize_ms=round(t_fk[0], 3), finalize_torch_ms=round(t_ft[0], 3))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["backbone", "forward", "patches", "all"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--patch-iters", type=int, default=3)
    ap.add_argument("--patch-batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT = args.out
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_seg_cnn.py measures on the GPU; none found")
    emit(bench="device", name=torch.cuda.get_device_name(0))
    for what, fn in (("backbone", bench_backbone), ("forward", bench_forward), ("patches", bench_patches)):
        if args.what in (what, "all"):
            fn(args)


if __name__ == "__main__":
    main()
