#!/usr/bin/env python3
"""The measurements of the weight EMA (profiles/ema.txt) on the C3 model (256 x 256, 16 images).  Not a test.

  python tools/ema_bench.py kernel [--out FILE]
      (a) one `ops.ema_update` launch over every parameter and floating buffer of the MetaGeneratorModel;
      (b) the obvious library alternative on the same tensors: `torch._foreach_lerp_` on the parameters plus
          `torch._foreach_copy_` on the buffers, into shadows laid out like the tensors;
      (c) the bytes (a) moves — 12 per averaged float (read p, read e, write e), 8 per copied float — over its time, as a
          share of the device-to-device copy rate measured in the same run (`copy_` of a buffer of the same number of bytes,
          8 bytes per float).
      (a) and (b) alternate, window by window.  Acceptance: (a) is not slower than (b).

  python tools/ema_bench.py steps [--ema_decay D] [--root DIR] [--out FILE]
      ms per training step of the C3 trainer, eager and replayed from HIP graphs, with `--ema_decay D` (0: off).
      `--root DIR` imports the package from another checkout: run it on a checkout of the parent commit for the figures
      from before the feature (that tree ignores --ema_decay).  Reported, not gated.

Timing: HIP events around a window of calls after untimed warm-up calls, several windows, the median and all values
reported.  Seeded synthetic batches; the weights are the initialisation (the kernels' work does not depend on the values).
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


def c3_trainer(T, synth, dev, ema_decay):
    base = synth.BASELINE_CONFIGS["C3"]
    vocab = synth.make_vocab(base["vocab"])
    opt = T.make_opt(vocab, ["--image_size", "256,256", "--no_vgg_loss", "--batch_size", "16"])
    opt.ema_decay = float(ema_decay)
    torch.manual_seed(0)
    tr = T.Trainer(opt, dev)
    cfg = base["cfg"]
    bs = [[None if t is None else t.to(dev) for t in
           synth.make_batch(vocab, synth.BatchConfig(16, 256, cfg.min_objects, cfg.max_objects, cfg.graph), seed=i)] for i in range(4)]
    return tr, bs


def kernel(args, dev):
    from canonicalsg2im_amd import ops, synth, train as T
    from canonicalsg2im_amd.ema import WeightEMA
    tr, _ = c3_trainer(T, synth, dev, 0.0)
    model = tr.model
    ema = WeightEMA(model, 0.999)
    table = ema.table
    n_avg = sum(n for n, k in zip(table.numels, table.kinds) if k == ops.EMA_AVERAGE)
    n_copy = sum(n for n, k in zip(table.numels, table.kinds) if k == ops.EMA_COPY)
    nbytes = 12 * n_avg + 8 * n_copy
    params = [p.detach() for p in model.parameters()]
    bufs = [b.detach() for b in model.buffers() if b.is_floating_point()]
    sh_p, sh_b = [torch.empty_like(p).copy_(p) for p in params], [torch.empty_like(b).copy_(b) for b in bufs]
    w = 1.0 - 0.999

    def ours():
        ops.ema_update(table, 0.999)

    def library():
        torch._foreach_lerp_(sh_p, params, w)
        if bufs:
            torch._foreach_copy_(sh_b, bufs)

    src = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    for fn in (ours, library, copy):
        for _ in range(args.warmup):
            fn()
    a, b, c = [], [], []
    for _ in range(args.windows):            # alternating: a drift of the device shows in all three alike
        a.append(window(ours, args.iters))
        b.append(window(library, args.iters))
        c.append(window(copy, args.iters))
    rate = nbytes / (median(a) * 1e-3) / 1e12
    copy_rate = nbytes / (median(c) * 1e-3) / 1e12
    lines = [
        "device: %s; C3 model (256 x 256): %d tensors in the table (%d chunks of %d floats), %d averaged floats (parameters), "
        "%d copied floats (floating buffers)" % (torch.cuda.get_device_name(0), table.n, table.chunks, ops.EMA_CHUNK, n_avg, n_copy),
        "HIP events, %d calls per window after %d warm-up calls, %d windows alternating (a), (b), copy; median [all windows]" % (
            args.iters, args.warmup, args.windows),
        "(a) ops.ema_update, ONE launch:                         %s per call" % fmt(a),
        "(b) torch._foreach_lerp_ + torch._foreach_copy_:        %s per call" % fmt(b),
        "    (a) / (b) = %.3f  -> (a) is %s than (b)" % (median(a) / median(b), "NOT slower" if median(a) <= median(b) else "SLOWER"),
        "(c) bytes moved by (a): 12 x %d + 8 x %d = %.1f MB -> %.2f TB/s" % (n_avg, n_copy, nbytes / 1e6, rate),
        "    device-to-device copy_ of the same number of bytes:  %s per call = %.2f TB/s (read + write)" % (fmt(c), copy_rate),
        "    (a) runs at %.1f %% of that copy rate" % (100.0 * rate / copy_rate),
    ]
    return lines


def steps(args, dev):
    from canonicalsg2im_amd import synth, train as T
    tr, bs = c3_trainer(T, synth, dev, args.ema_decay)
    has_ema = getattr(tr, "ema", None) is not None
    it = [0]

    def step():
        tr.step(bs[it[0] % 4])
        it[0] += 1

    for _ in range(10):                      # eager, the set's capture, the encoder buckets' captures, replays
        step()
    replayed = [window(step, args.iters) for _ in range(args.windows)]
    replays = tr.graphs.replays if tr.graphs is not None else 0
    tr.use_graphs = False
    for _ in range(3):
        step()
    eager = [window(step, args.iters) for _ in range(args.windows)]
    return ["device: %s; tree %s; C3 trainer (256 x 256, 16 images, --no_vgg_loss), --ema_decay %g: EMA %s%s" % (
                torch.cuda.get_device_name(0), args.shown, args.ema_decay, "ON" if has_ema else "off",
                ", %d updates" % tr.ema.num_updates if has_ema else ""),
            "HIP events, %d steps per window, %d windows; median [all windows]" % (args.iters, args.windows),
            "replayed step (%d replays so far): %s per step" % (replays, fmt(replayed)),
            "eager step:                        %s per step" % fmt(eager)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "steps"])
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ema_decay", type=float, default=0.0)
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.iters is None:
        args.iters = 50 if args.what == "kernel" else 10
    args.shown = args.root or "this checkout"
    sys.path.insert(0, os.path.abspath(args.root or HERE))
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_bench.py measures on the device: no HIP device here, nothing measured")
    dev = torch.device("cuda", 0)
    lines = kernel(args, dev) if args.what == "kernel" else steps(args, dev)
    text = "\n".join(["$ python tools/ema_bench.py " + " ".join(sys.argv[1:] if argv is None else argv)] + lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
