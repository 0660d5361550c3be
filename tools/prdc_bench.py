#!/usr/bin/env python3
"""The measurement of the k-nearest-neighbour manifold entries (profiles/prdc.txt), synthetic features:

  ops.knn_radii and ops.ball_counts at (n, m, D, k) = (10000, 10000, 2048, 5) and, if memory allows, (50000, 50000, 2048, 5):
  ms per entry for the four calls behind precision / recall / density / coverage — radii(real), radii(gen),
  ball_counts(gen, real), ball_counts(real, gen) —, the fp64 rate over the tiles' operations (three per pair and column: a
  subtraction, a product, a sum) and the peak device memory above the features.  At 10000 also torch's fp64 materialising
  version (cdist, kthvalue, compare) with its time and peak memory, and whether the four numbers are equal.

    python tools/prdc_bench.py [--iters 3] [--warmup 1] [--out profiles/prdc.txt]

Recorded numbers, not gates.  Timing: HIP events around `iters` calls after `warmup` untimed ones, three times; the median
is reported with the three values.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


LATENT = 16


def features(n, m, D, dev):
    """Rows on a LATENT-dimensional subspace of the D columns: standard normal real rows and normal + 0.3 generated rows in
    an orthonormal basis of it, rounded to fp32.  Their distances are those of 16-dimensional rows, so all four numbers lie
    strictly inside (0, 1) and the comparison with torch says something about each; D independent columns give precision 1,
    recall 0 and coverage 1 at these sizes.  The kernels' work does not depend on the values."""
    g = torch.Generator().manual_seed(1)
    basis = torch.linalg.qr(torch.randn(D, LATENT, generator=g, dtype=torch.float64)).Q.T
    real = (torch.randn(n, LATENT, generator=g, dtype=torch.float64) @ basis).float().to(dev)
    gen = ((torch.randn(m, LATENT, generator=g, dtype=torch.float64) + 0.3) @ basis).float().to(dev)
    return real, gen


def peak_above(fn):
    """-> (fn's result, the peak of allocated device memory during fn above what was allocated before it, MiB)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def torch_prdc(real, gen, k):
    """The obvious way: three fp64 distance matrices in memory, kthvalue (k + 1: the row itself is in its own matrix at 0),
    compare."""
    x, y = real.double(), gen.double()
    r_real = torch.cdist(x, x).kthvalue(k + 1, dim=1).values
    r_gen = torch.cdist(y, y).kthvalue(k + 1, dim=1).values
    d = torch.cdist(x, y)                                  # (n_real, n_gen)
    in_real = d <= r_real[:, None]                         # [i, j]: generated j inside the ball of real i
    in_gen = d <= r_gen[None, :]
    inside = in_real.sum(dim=0)
    sums = torch.stack([(inside > 0).sum(), in_gen.any(dim=1).sum(), inside.sum(), in_real.any(dim=1).sum()]).cpu().tolist()
    n_real, n_gen = x.shape[0], y.shape[0]
    return {"precision": sums[0] / n_gen, "recall": sums[1] / n_real, "density": sums[2] / (k * n_gen),
            "coverage": sums[3] / n_real, "k": k, "n": [n_real, n_gen]}


def one_size(ops, quality, n, m, D, k, dev, iters, warmup, with_torch):
    real, gen = features(n, m, D, dev)
    r_real, r_gen = ops.knn_radii(real, k), ops.knn_radii(gen, k)
    entries = [("knn_radii(real)", lambda: ops.knn_radii(real, k), n, n),
               ("knn_radii(gen)", lambda: ops.knn_radii(gen, k), m, m),
               ("ball_counts(gen, real)", lambda: ops.ball_counts(gen, real, r_real), m, n),
               ("ball_counts(real, gen)", lambda: ops.ball_counts(real, gen, r_gen), n, m)]
    lines = ["", "(n, m, D, k) = (%d, %d, %d, %d):" % (n, m, D, k)]
    total = 0.0
    for name, fn, rows, cols in entries:
        t = timed(fn, iters, warmup)
        tiles = -(-rows // 64) * -(-cols // 64)
        rate = tiles * 64 * 64 * D * 3.0 / (t[1] * 1e-3) / 1e12
        total += t[1]
        lines.append("  %-24s %9.2f ms per call  %s  = %.2f TFLOP/s fp64 over %d tiles (sub, mul, add per pair and column)" % (
            name, t[1], ["%.2f" % v for v in t], rate, tiles))
    ours, peak = peak_above(lambda: quality.prdc_from_features(real, gen, k))
    lines += ["  the four entries together %8.2f ms; prdc_from_features: peak device memory %.1f MiB above the features" % (total, peak),
              "  %s" % {key: ours[key] for key in ("precision", "recall", "density", "coverage")}]
    if with_torch:
        t = timed(lambda: torch_prdc(real, gen, k), iters, warmup)
        theirs, peak = peak_above(lambda: torch_prdc(real, gen, k))
        lines += ["  torch fp64 cdist + kthvalue + compare (three n x m matrices in memory) %9.2f ms per call  %s; peak %.1f MiB" % (
            t[1], ["%.2f" % v for v in t], peak),
                  "  %s" % {key: theirs[key] for key in ("precision", "recall", "density", "coverage")},
                  "  the four numbers of the two are %s" % ("EQUAL" if theirs == ours else "NOT equal")]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from canonicalsg2im_amd import ops, quality
    dev = torch.device("cuda", 0)
    lines = ["device: %s; synthetic features (normal rows on a 16-dimensional subspace); HIP events, %d calls per window after %d warm-up calls, median of 3"
             % (torch.cuda.get_device_name(0), args.iters, args.warmup)]
    lines += one_size(ops, quality, 10000, 10000, 2048, 5, dev, args.iters, args.warmup, with_torch=True)
    torch.cuda.empty_cache()
    try:
        lines += one_size(ops, quality, 50000, 50000, 2048, 5, dev, args.iters, args.warmup, with_torch=False)
    except torch.cuda.OutOfMemoryError:
        lines += ["", "(n, m, D, k) = (50000, 50000, 2048, 5): left out, the device's memory does not allow it"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
