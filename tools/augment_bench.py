#!/usr/bin/env python3
"""The measurements of DiffAugment (profiles/d_augment.txt).  Not a test; no figure is fixed in advance.

  python tools/augment_bench.py kernel [--out FILE]
      Forward (`ops.d_augment`) and backward (the adjoint launch of its autograd Function), all three policies on, (a) on the C3 packed PatchGAN input
      (16 x 256 x 256 x 40 fp32, c0 = 32) and (b) on 128 crops (128 x 32 x 32 x 4, c0 = 0), against the yardstick: a
      `copy_` of the same buffer, timed in the same process, window by window in turn.  With colour on the forward reads
      its input twice (the per-sample sum, then the map) and writes once, so it cannot beat the copy: the ratio is
      recorded, not promised.  Also the two policies that move no colour (translation,cutout): one read, one write.

  python tools/augment_bench.py steps [--out FILE]
      ms per training step of the C3 trainer, replayed from HIP graphs, with `--d_augment color,translation,cutout` against
      off: ONE trainer switched between the two (same allocations; each leg replays its own captured graph set), same
      process, same build, windows in turn.  The difference is recorded in ms.

  python tools/augment_bench.py ada [--out FILE]
      The adaptive strength (profiles/d_augment_ada.txt).  (a) The GATED forward and backward on the C3 packed input, all
      three policies, with the gate filled on the device at p24 = 2^24 (every sample on) and at 2^23 (each policy on half
      of the samples), against the UNGATED kernels of the same build, windows in turn; the spread of the ungated figure
      over the windows is reported beside the difference.  (b) What an adaptive run adds to a step: `ada_accumulate` over
      the C3 recipe's two prediction maps, plus one `ada_update` and the three gate fills of `begin_step`.

  python tools/augment_bench.py pipeline [--out FILE]
      The ADA pipeline (profiles/ada_pipeline.txt): forward (`ops.ada_pipeline`'s launch) and backward (its adjoint) on the C3
      packed input with rows filled on the device at p = 1 for all three groups, for blitting alone (the copy path), and for
      the row with the largest search box among 10^4 generated keys (every sample given that row); beside them, windows in
      turn, a `copy_` of the same buffer and DiffAugment's forward and backward; and the three table fills of `begin_step`.

Timing: HIP events around a window of calls after untimed warm-up calls, several windows, the median and all values
reported.  Seeded inputs; the kernels' work does not depend on the values.
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def fmt(v):
    return "%.4f ms  [%s]" % (median(v), " ".join("%.4f" % x for x in v))


def kernel(args, dev):
    from canonicalsg2im_amd import ops
    lines = ["device: %s; HIP events, %d calls per window after %d warm-up calls, %d windows in turn; median [all windows]" % (
        torch.cuda.get_device_name(0), args.iters, args.warmup, args.windows)]
    for name, (N, H, Ct, c0) in (("C3 packed PatchGAN input", (16, 256, 40, 32)), ("128 crops", (128, 32, 4, 0))):
        torch.manual_seed(0)
        x = ops.empty_nhwc(N, Ct, H, H, dev).normal_()
        g = ops.empty_nhwc(N, Ct, H, H, dev).normal_()
        dst = torch.empty_like(x)
        table = ops.augment_table(0, 1, 0, N, H, device=dev)
        nbytes = x.numel() * 4
        runs = {}
        for label, policy in (("color,translation,cutout", 7), ("translation,cutout", 6)):
            runs[label + " forward"] = lambda policy=policy: ops.d_augment(x, table, c0, policy)
            # the adjoint as the Function's backward issues it (ops._aug_launch on a gradient that is already there): timed
            # through autograd the call is bound by the host, 0.07-0.08 ms whatever the size
            runs[label + " backward"] = lambda policy=policy: ops._aug_launch("diff", True, g, table, c0, policy)
        runs["copy_ of the same buffer"] = lambda: dst.copy_(x)
        for fn in runs.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in runs}
        for _ in range(args.windows):
            for k, fn in runs.items():
                times[k].append(window(fn, args.iters))
        copy = median(times["copy_ of the same buffer"])
        lines.append("%s: %d x %d x %d x %d fp32 = %.1f MB, c0 = %d" % (name, N, H, H, Ct, nbytes / 1e6, c0))
        for k, v in times.items():
            lines.append("    %-42s %s per call = %.2f x the copy, %.2f TB/s of (one read + one write)" % (
                k, fmt(v), median(v) / copy, 2 * nbytes / (median(v) * 1e-3) / 1e12))
    return lines


def ada(args, dev):
    from canonicalsg2im_amd import ops
    lines = ["device: %s; HIP events, %d calls per window after %d warm-up calls, %d windows in turn; median [all windows]" % (
        torch.cuda.get_device_name(0), args.iters, args.warmup, args.windows)]
    N, H, Ct, c0 = 16, 256, 40, 32
    torch.manual_seed(0)
    x = ops.empty_nhwc(N, Ct, H, H, dev).normal_()
    g = ops.empty_nhwc(N, Ct, H, H, dev).normal_()
    table = ops.augment_table(0, 1, 0, N, H, device=dev)
    gates = {}
    for label, p24 in (("p24 = 2^24", 1 << 24), ("p24 = 2^23", 1 << 23)):
        ctrl = torch.tensor([p24, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
        gates[label] = ops.augment_gate(0, 1, 0, N, ctrl)
    runs = {"ungated forward": lambda: ops.d_augment(x, table, c0, 7),
            "ungated backward": lambda: ops._aug_launch("diff", True, g, table, c0, 7)}
    for label, gate in gates.items():
        runs["gated forward,  " + label] = lambda gate=gate: ops.d_augment(x, table, c0, 7, gate=gate)
        runs["gated backward, " + label] = lambda gate=gate: ops._aug_launch("gated", True, g, table, c0, 7, gate)
    # the C3 recipe's PatchGAN: two scales, 16 pictures, prediction maps of 35 x 35 and 19 x 19 (4 x 4 convolutions, three
    # of stride 2, on 256 and 128 pixels)
    preds = [torch.randn(16, 1, 35, 35, device=dev), torch.randn(16, 1, 19, 19, device=dev)]
    ctrl = torch.zeros(8, dtype=torch.int64, device=dev)
    three = torch.zeros((3, N), dtype=torch.int32, device=dev)
    runs["ada_accumulate, 2 maps of 16 pictures"] = lambda: ops.ada_accumulate(preds, ctrl)
    runs["ada_update"] = lambda: ops.ada_update(ctrl, 10066330, 537)
    runs["three gate fills of 16 rows"] = lambda: [ops.augment_gate(0, 1, p, N, ctrl, out=three[p]) for p in range(3)]
    for fn in runs.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in runs}
    for _ in range(args.windows):
        for k, fn in runs.items():
            times[k].append(window(fn, args.iters))
    lines.append("C3 packed PatchGAN input: %d x %d x %d x %d fp32 = %.1f MB, c0 = %d, color,translation,cutout; gate masks at 2^23: %s" % (
        N, H, H, Ct, x.numel() * 4 / 1e6, c0, gates["p24 = 2^23"].tolist()))
    for k, v in times.items():
        base = times.get("ungated " + ("forward" if "forward" in k else "backward")) if k.startswith("gated") else None
        tail = "" if base is None else "  = %+.4f ms against ungated (ungated windows span %.4f ms)" % (
            median(v) - median(base), max(base) - min(base))
        lines.append("    %-42s %s per call%s" % (k, fmt(v), tail))
    return lines


def pipeline(args, dev):
    from canonicalsg2im_amd import ops
    lines = ["device: %s; HIP events, %d calls per window after %d warm-up calls, %d windows in turn; median [all windows]" % (
        torch.cuda.get_device_name(0), args.iters, args.warmup, args.windows)]
    N, H, Ct, c0 = 16, 256, 40, 32
    torch.manual_seed(0)
    x = ops.empty_nhwc(N, Ct, H, H, dev).normal_()
    g = ops.empty_nhwc(N, Ct, H, H, dev).normal_()
    dst = torch.empty_like(x)
    ctrl = torch.tensor([1 << 24, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
    tables = {"blit,geom,color at p = 1": ops.ada_pipeline_table(0, 1, 0, N, H, 56, ctrl),
              "blit alone at p = 1 (copies)": ops.ada_pipeline_table(0, 1, 0, N, H, 8, ctrl)}
    host = ops.ada_pipeline_table_host(0, 1, 0, 10000, H, 56, 1 << 24)
    G = host[:, 6:12].view(torch.float32).abs().double()
    half = torch.maximum(G[:, 0] + G[:, 1], G[:, 3] + G[:, 4])
    worst = int(half.argmax())
    tables["largest box of 10^4 keys (row %d, half side %.3f)" % (worst, float(half[worst]))] = host[worst:worst + 1].repeat(N, 1).to(dev)
    old = ops.augment_table(0, 1, 0, N, H, device=dev)
    three = torch.zeros((3, N, 32), dtype=torch.int32, device=dev)
    runs = {}
    for label, t in tables.items():
        runs[label + ": forward"] = lambda t=t: ops._aug_launch("ada", False, x, t, c0)
        runs[label + ": backward"] = lambda t=t: ops._aug_launch("ada", True, g, t, c0)
    runs["copy_ of the same buffer"] = lambda: dst.copy_(x)
    runs["d_augment color,translation,cutout: forward"] = lambda: ops.d_augment(x, old, c0, 7)
    runs["d_augment color,translation,cutout: backward"] = lambda: ops._aug_launch("diff", True, g, old, c0, 7)
    runs["three table fills of 16 rows"] = lambda: [ops.ada_pipeline_table(0, 1, p, N, H, 56, ctrl, out=three[p]) for p in range(3)]
    for fn in runs.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in runs}
    for _ in range(args.windows):
        for k, fn in runs.items():
            times[k].append(window(fn, args.iters))
    copy = median(times["copy_ of the same buffer"])
    lines.append("C3 packed PatchGAN input: %d x %d x %d x %d fp32 = %.1f MB, c0 = %d" % (N, H, H, Ct, x.numel() * 4 / 1e6, c0))
    for k, v in times.items():
        lines.append("    %-62s %s per call = %.2f x the copy" % (k, fmt(v), median(v) / copy))
    return lines


def c3_trainer(T, synth, dev, policies):
    base = synth.BASELINE_CONFIGS["C3"]
    vocab = synth.make_vocab(base["vocab"])
    opt = T.make_opt(vocab, ["--image_size", "256,256", "--no_vgg_loss", "--batch_size", "16", "--d_augment", policies])
    torch.manual_seed(0)
    tr = T.Trainer(opt, dev)
    cfg = base["cfg"]
    bs = [[None if t is None else t.to(dev) for t in
           synth.make_batch(vocab, synth.BatchConfig(16, 256, cfg.min_objects, cfg.max_objects, cfg.graph), seed=i)] for i in range(4)]
    return tr, bs


def steps(args, dev):
    from canonicalsg2im_amd import synth, train as T
    tr, bs = c3_trainer(T, synth, dev, "color,translation,cutout")
    aug, it = tr.d_augment, [0]

    def switch(on):
        # ONE trainer, so that both legs run on the same allocations: off = the DAugment object taken away, which is what a
        # trainer without the flag holds (None); the policy is part of the graph key, so each leg has its own captured set
        obj = aug if on else None
        tr.d_augment = tr.discriminator.img_discriminator.d_augment = tr.discriminator.obj_discriminator.d_augment = obj

    def step():
        tr.step(bs[it[0] % 4])
        it[0] += 1

    for on in (False, True):
        switch(on)
        for _ in range(10):                  # eager, the set's capture, the encoder buckets' captures, replays
            step()
    times = {False: [], True: []}
    for _ in range(args.windows):
        for on in (False, True):
            switch(on)
            times[on].append(window(step, args.iters))
    return ["device: %s; C3 trainer (256 x 256, 16 images, --no_vgg_loss), replayed path, ONE trainer switched between the legs" %
            torch.cuda.get_device_name(0),
            "HIP events, %d steps per window, %d windows in turn; median [all windows]; %d replays, %d eager steps, %d graph sets" % (
                args.iters, args.windows, tr.graphs.replays, tr._eager_steps, len(tr.graphs.sets)),
            "augmentation off:                      %s per step" % fmt(times[False]),
            "color,translation,cutout:              %s per step" % fmt(times[True]),
            "difference: %+.3f ms per step" % (median(times[True]) - median(times[False]))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "steps", "ada", "pipeline"])
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.iters is None:
        args.iters = 10 if args.what == "steps" else 200 if args.what == "pipeline" else 2000        # kernel windows of 0.04-0.2 s
    sys.path.insert(0, HERE)
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_bench.py measures on the device: no HIP device here, nothing measured")
    dev = torch.device("cuda", 0)
    lines = {"kernel": kernel, "steps": steps, "ada": ada, "pipeline": pipeline}[args.what](args, dev)
    text = "\n".join(["$ python tools/augment_bench.py " + " ".join(sys.argv[1:] if argv is None else argv)] + lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
