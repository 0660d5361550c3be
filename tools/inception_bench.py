#!/usr/bin/env python3
"""Throughput of the Inception-v3 forward with the STAND-IN weights: img/s at batch 50 from 299 x 299 and 256 x 256 uint8
sources, both variants, and the kernel split of one pass from the library's per-kernel events (csg_prof_*).

    python tools/inception_bench.py [--batch 50] [--iters 10] [--warmup 3] [--out profiles/inception_bench.json]

A recorded number, not a gate: nothing earlier exists to compare it with.  Timing: HIP events around `iters` passes after
`warmup` untimed ones, repeated three times; the median is reported with the three values.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from canonicalsg2im_amd import _lib, inception          # the built library (python -c "import __graft_entry__ as g; g.build()")
    dev = torch.device("cuda", 0)
    result = {"weights": "stand-in (random)", "batch": args.batch, "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "runs": []}
    for variant in ("torchvision", "fid"):
        net = inception.InceptionV3(variant, "random").to(dev)
        for side in (299, 256):
            pics = torch.randint(0, 256, (args.batch, side, side, 3), dtype=torch.uint8,
                                 generator=torch.Generator().manual_seed(side)).to(dev)

            def one_pass():
                return net(inception.prepare(pics, variant))

            for _ in range(args.warmup):
                one_pass()
            rates = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.iters):
                    one_pass()
                e1.record()
                torch.cuda.synchronize()
                rates.append(args.batch * args.iters / (e0.elapsed_time(e1) / 1e3))
            _lib.prof_reset()
            _lib.prof_enable(1)
            one_pass()
            torch.cuda.synchronize()
            split = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in sorted(_lib.prof_read().items(), key=lambda kv: -kv[1][0])}
            _lib.prof_enable(0)
            row = {"variant": variant, "source": "%dx%d uint8" % (side, side), "img_per_s": round(sorted(rates)[1], 1),
                   "img_per_s_runs": [round(r, 1) for r in rates], "kernel_ms_one_pass": split,
                   "kernel_ms_total": round(sum(v["ms"] for v in split.values()), 3)}
            result["runs"].append(row)
            print("%-12s %s: %.1f img/s %s; kernels of one pass %.2f ms" % (variant, row["source"], row["img_per_s"],
                                                                            row["img_per_s_runs"], row["kernel_ms_total"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))
    return result


if __name__ == "__main__":
    main()
