#!/usr/bin/env python3
"""The two measurements of KID and the object-level FID (profiles/quality_objects.txt), STAND-IN weights:

  1. ops.kid_sums at (S, m, D) = (100, 1000, 2048): time per call, and beside it the torch expression
     ((a @ b.T) * gamma + coef0) ** 3 with .sum() in float64 on the device for the same subsets (it materialises the three
     m x m matrices per subset); the two results are compared.
  2. crops per second of crop + Inception forward at batch 50 (ObjectFID.features, 4 boxes on each of 50 pictures of
     256 x 256, 200 crops), and beside it the pictures per second of FID.features on the same pictures.

    python tools/quality_objects_bench.py [--iters 5] [--warmup 2] [--out profiles/quality_objects.txt]

Recorded numbers, not gates.  Timing: HIP events around `iters` calls after `warmup` untimed ones, three times; the median
is reported with the three values.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters, warmup):
    """-> the three per-call times in ms, sorted."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return sorted(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from canonicalsg2im_amd import inception, ops, quality
    dev = torch.device("cuda", 0)
    lines = ["device: %s; weights: stand-in (random); HIP events, %d calls per window after %d warm-up calls, median of 3"
             % (torch.cuda.get_device_name(0), args.iters, args.warmup)]

    # ---- 1. kid_sums
    S, m, D, n = 100, 1000, 2048, 5000
    g = torch.Generator().manual_seed(1)
    fx = torch.randn(n, D, generator=g).abs().to(dev)
    fy = (torch.randn(n, D, generator=g) + 0.3).abs().to(dev)
    rng = np.random.RandomState(0)
    ix = torch.from_numpy(np.stack([rng.choice(n, m, replace=False) for _ in range(S)]).astype(np.int32)).to(dev)
    iy = torch.from_numpy(np.stack([rng.choice(n, m, replace=False) for _ in range(S)]).astype(np.int32)).to(dev)
    gamma = 1.0 / D

    def hip():
        return ops.kid_sums(fx, fy, ix, iy, gamma, 1.0, 3)

    def eager():
        out = torch.empty(S, 3, device=dev, dtype=torch.float64)
        for s in range(S):
            X, Y = fx[ix[s].long()].double(), fy[iy[s].long()].double()
            kxx, kyy, kxy = (((a @ b.T) * gamma + 1.0) ** 3 for a, b in ((X, X), (Y, Y), (X, Y)))
            out[s, 0] = kxx.sum() - kxx.diagonal().sum()
            out[s, 1] = kyy.sum() - kyy.diagonal().sum()
            out[s, 2] = kxy.sum()
        return out

    t_hip, t_eager = timed(hip, args.iters, args.warmup), timed(eager, args.iters, args.warmup)
    a, b = hip(), eager()
    rel = float(((a - b).abs() / b.abs()).max())
    tiles = 100 * (16 * 17 + 16 * 16)
    flops = tiles * 64 * 64 * D * 2.0
    lines += ["",
              "kid_sums (S, m, D) = (%d, %d, %d), features of %d rows per side:" % (S, m, D, n),
              "  hand-written (csg_kid_sums, fixed summation order)   %8.2f ms per call  %s" % (t_hip[1], ["%.2f" % t for t in t_hip]),
              "    = %.2f TFLOP/s fp64 over the %d tiles' multiply-adds (vector FMA; no matrix cores)" % (
                  flops / (t_hip[1] * 1e-3) / 1e12, tiles),
              "  torch fp64 matmul + pow + sum (materialises 3 m x m)   %8.2f ms per call  %s" % (t_eager[1], ["%.2f" % t for t in t_eager]),
              "  largest relative difference of the %d sums: %.2e" % (3 * S, rel)]

    # ---- 2. crops + Inception forward, beside whole pictures
    net = inception.InceptionV3("fid", "random").to(dev)
    pics = torch.randint(0, 256, (50, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(dev)
    brng = np.random.RandomState(3)
    boxes = np.concatenate([brng.uniform(0, 0.6, (200, 2)), brng.uniform(0.1, 0.4, (200, 2))], axis=1).astype(np.float32)
    boxes_dev = torch.from_numpy(boxes).to(dev)
    index_dev = torch.arange(50, dtype=torch.int32).repeat_interleave(4).to(dev)
    ofid = quality.ObjectFID(net, batch_size=50)
    fid = quality.FID(net)
    t_crops = timed(lambda: ofid.features(pics, boxes_dev, index_dev), args.iters, args.warmup)
    t_pics = timed(lambda: fid.features(pics), args.iters, args.warmup)
    t_stage = timed(lambda: ops.crop_resize_bilinear(pics, ops.crop_windows(boxes_dev, 256, 256)[:50], index_dev[:50],
                                                     (299, 299), 2.0, -1.0), args.iters, args.warmup)
    t_prepare = timed(lambda: inception.prepare(pics, "fid"), args.iters, args.warmup)
    lines += ["",
              "crop + Inception forward, 2048-wide features, batch 50 (200 crops of 50 pictures of 256 x 256):",
              "  ObjectFID.features   %8.1f crops/s     %s ms per 200 crops" % (200 / (t_crops[1] * 1e-3), ["%.1f" % t for t in t_crops]),
              "  FID.features         %8.1f pictures/s  %s ms per 50 pictures" % (50 / (t_pics[1] * 1e-3), ["%.1f" % t for t in t_pics]),
              "  the input stages alone, 50 maps of 299 x 299: crop_windows + crop_resize_bilinear %.3f ms, prepare %.3f ms" % (
                  t_stage[1], t_prepare[1])]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
