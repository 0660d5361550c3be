#!/usr/bin/env python3
"""Time the split walk over a seeded COCO-shaped folder, three forms over the same batches:

    device   the builder's batches through the two `Sampler.generate` calls and the `gt` deprocess; nothing copied or written
    serial   the same, then `.cpu()` and `Image.save` for each picture in the loop's thread: what scripts/sample.py did before
             the split walk existed, with only the calls that existed then
    split    `split.generate_split` with --num_writers threads (pinned double buffer, side-stream copies, writer pool)

    python tools/split_speed.py folder DIR                       write the folder (host only)
    python tools/split_speed.py device|serial|split DIR [--out OUT] [--num_writers 8]
                                                                 one form, one process -> one JSON line
    python tools/split_speed.py count DIR                        the package's launches of one eager batch, per kernel
    python tools/split_speed.py same OUT_A OUT_B                 are the pictures of two runs the same bytes?
    python tools/split_speed.py all DIR [--rounds 3] [--report FILE]
                                                                 folder, then alternating fresh processes, then the report

The folder: 256 JPEGs of 480 x 640 generated from a seed (smooth noise, so they decode like photographs rather than like
static), 8 objects each (6 things, 2 stuff), <DIR>/MSCoco in the reference's layout; nothing from outside the tree.  The
model: C3 shapes — 256 x 256, batch 16, `--dataset coco` — with freshly initialised weights (seed 0), 16 loader threads.
Every form first walks three batches of its own form (eager, capturing, replayed: every replay key of the timed pass),
then the timed pass of all 16, ended by a device synchronise (and, for `split`, by the writer's close, which is inside
generate_split).  img/s = 256 / that wall-clock time."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, THINGS, STUFF = 256, 480, 640, 6, 2
SETS = ("gt", "generation/gt_box_gt_mask", "generation/pred_box_pred_mask")


def write_folder(root):
    import numpy as np
    from PIL import Image
    base = os.path.join(root, "MSCoco")
    image_dir = os.path.join(base, "images", "val2017")
    os.makedirs(image_dir, exist_ok=True)
    os.makedirs(os.path.join(base, "annotations"), exist_ok=True)
    cats = {"instances": [{"id": i, "name": "thing_%d" % i} for i in range(1, 81)],
            "stuff": [{"id": i, "name": "stuff_%d" % i} for i in range(92, 183)]}
    images, ann = [], {"instances": [], "stuff": []}
    for k in range(N):
        rng = np.random.default_rng(7000 + k)
        image_id = 1000 + k
        coarse = rng.integers(0, 256, size=(15, 20, 3), dtype=np.uint8)
        im = Image.fromarray(coarse, "RGB").resize((W, H), Image.BICUBIC)
        px = np.asarray(im).astype(np.int16) + rng.integers(-6, 7, size=(H, W, 3))
        name = "%012d.jpg" % image_id
        Image.fromarray(np.clip(px, 0, 255).astype(np.uint8), "RGB").save(os.path.join(image_dir, name), quality=90)
        images.append({"id": image_id, "file_name": name, "width": W, "height": H})
        for j in range(THINGS + STUFF):
            kind = "instances" if j < THINGS else "stuff"
            w, h = float(rng.uniform(0.2, 0.5) * W), float(rng.uniform(0.2, 0.5) * H)      # every box above 2% of the picture
            x, y = float(rng.uniform(0, W - w)), float(rng.uniform(0, H - h))
            cat = cats[kind][int(rng.integers(0, len(cats[kind])))]["id"]
            ann[kind].append({"id": image_id * 100 + j, "image_id": image_id, "category_id": cat, "bbox": [x, y, w, h],
                              "segmentation": []})
    for kind in ("instances", "stuff"):
        with open(os.path.join(base, "annotations", "%s_val2017.json" % kind), "w") as f:
            json.dump({"images": images, "categories": cats[kind], "annotations": ann[kind]}, f)
    return image_dir


def setup(root, loader_threads=16):
    import torch

    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.scripts.train import build_parser, folder_dataset
    argv = ["--image_size", "256,256", "--no_vgg_loss", "--use_img_disc", "0", "--batch_size", "16", "--dataset", "coco",
            "--dataroot", root, "--loader_num_workers", str(loader_threads)]
    ds = folder_dataset(build_parser().parse_args(argv), "val")
    if ds is None or len(ds) != N:
        raise SystemExit("split_speed: %s holds no folder of %d pictures (run the `folder` mode first)" % (root, N))
    opt = T.make_opt(ds.vocab, argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    return ds, opt, dev, Sampler(opt, dev)


def batches(ds, opt, sampler, dev, count=None):
    from canonicalsg2im_amd.scripts.train import folder_builder
    from canonicalsg2im_amd.sg2im.data.loader import file_order_batches
    lists = file_order_batches(len(ds), opt.batch_size)[:count]
    builder = folder_builder(ds, opt, sampler, dev, rng=random.Random(0))
    try:
        yield from builder.batches(lists)
    finally:
        builder.close()


def walk(sampler, batch):
    """The device work of one batch, with the calls the parent commit has -> {set: uint8 (B,3,H,W)}."""
    import torch

    from canonicalsg2im_amd import ops
    imgs, objs, boxes, triplets, _, tt, masks, _ = batch
    with torch.no_grad():
        return {"generation/gt_box_gt_mask": sampler.generate(objs, triplets, tt, boxes_gt=boxes, masks_gt=masks)[0],
                "generation/pred_box_pred_mask": sampler.generate(objs, triplets, tt)[0],
                "gt": ops.deprocess_u8(imgs.float().contiguous(memory_format=torch.channels_last), True)}


def run_device(sampler, bs, out):
    done = 0
    for batch in bs:
        walk(sampler, batch)
        done += int(batch[1].shape[0])
    return done


def run_serial(sampler, bs, out):
    from PIL import Image
    for s in SETS:
        os.makedirs(os.path.join(out, *s.split("/")), exist_ok=True)
    done = 0
    for batch in bs:
        ids = batch[7].cpu().tolist()
        for s, t in walk(sampler, batch).items():
            host = t.permute(0, 2, 3, 1).contiguous().cpu().numpy()
            for i, image_id in enumerate(ids):
                Image.fromarray(host[i]).save(os.path.join(out, *s.split("/"), "%d.png" % image_id))
        done += len(ids)
    return done


def one_form(a):
    import torch
    ds, opt, dev, sampler = setup(a.dir)
    out = a.out or os.path.join(a.dir, "out_" + a.mode)
    if a.mode == "split":
        from canonicalsg2im_amd.split import generate_split

        def run(bs, where):
            return len(generate_split(sampler, bs, where, deprocess="imagenet", num_writers=a.num_writers)[1])
    else:
        run = (lambda bs, where: run_device(sampler, bs, where)) if a.mode == "device" else \
            (lambda bs, where: run_serial(sampler, bs, where))
    run(batches(ds, opt, sampler, dev, 3), out + "_warmup")
    torch.cuda.synchronize()
    before = (sampler.replays, sampler.eager_calls)
    t0 = time.perf_counter()
    done = run(batches(ds, opt, sampler, dev), out)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"mode": a.mode, "images": done, "seconds": round(dt, 4), "img_per_s": round(done / dt, 2),
                      "replays": sampler.replays - before[0], "eager_calls": sampler.eager_calls - before[1],
                      "num_writers": a.num_writers if a.mode == "split" else 0, "out": out}), flush=True)


def count_launches(a):
    import torch

    from canonicalsg2im_amd import _lib, graphs
    ds, opt, dev, sampler = setup(a.dir, 2)
    graphs.ENABLED = False
    bs = list(batches(ds, opt, sampler, dev, 2))
    walk(sampler, bs[0])
    torch.cuda.synchronize()
    _lib.prof_enable(1)
    _lib.prof_reset()
    walk(sampler, bs[1])
    torch.cuda.synchronize()
    table = {k: int(v[1]) for k, v in _lib.prof_read().items()}
    _lib.prof_enable(0)
    print(json.dumps({"mode": "count", "launches": sum(table.values()), "per_kernel": table}), flush=True)


def same_pictures(out_a, out_b):
    """-> (files compared, files that differ or are missing on one side)."""
    n = bad = 0
    for s in SETS:
        da, db = os.path.join(out_a, *s.split("/")), os.path.join(out_b, *s.split("/"))
        names = sorted(set(os.listdir(da)) | set(os.listdir(db)))
        for name in names:
            n += 1
            pa, pb = os.path.join(da, name), os.path.join(db, name)
            if not (os.path.isfile(pa) and os.path.isfile(pb)):
                bad += 1
                continue
            from PIL import Image
            import numpy as np
            with Image.open(pa) as ia, Image.open(pb) as ib:
                bad += int(ia.size != ib.size or not np.array_equal(np.asarray(ia), np.asarray(ib)))
    return n, bad


def child(mode, root, extra=(), limit=600):
    """One fresh process of this script -> its JSON line.  A child that fails or overruns ends the whole measurement."""
    cmd = [sys.executable, os.path.abspath(__file__), mode, root] + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("split_speed: `%s` ended with status %d; nothing further is run" % (" ".join(cmd[2:]), r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(xs):
    return max(xs) - min(xs)


def run_all(a):
    t0 = time.perf_counter()
    write_folder(a.dir)
    folder_s = time.perf_counter() - t0
    forms = ("device", "serial", "split")
    rounds = []
    for r in range(a.rounds):
        row = {}
        for mode in forms:                                 # alternating: every round runs each form once, in a fresh process
            row[mode] = child(mode, a.dir, ["--num_writers", str(a.num_writers)])
            print("round %d %s" % (r + 1, json.dumps(row[mode])), flush=True)
        rounds.append(row)
    n, bad = same_pictures(rounds[-1]["serial"]["out"], rounds[-1]["split"]["out"])
    count = child("count", a.dir)
    rate = {m: [row[m]["img_per_s"] for row in rounds] for m in forms}
    med = {m: sorted(v)[len(v) // 2] for m, v in rate.items()}
    lines = [
        "The split walk: generate_split against the serial form and the device alone",
        "==========================================================================",
        "",
        "tools/split_speed.py all, one MI355X, alternating fresh processes (device, serial, split) x %d rounds." % a.rounds,
        "%d seeded JPEGs of %d x %d, %d objects each; C3 shapes (256 x 256, batch 16, --dataset coco), fresh weights, 16 loader"
        % (N, H, W, THINGS + STUFF),
        "threads; three pictures per image (gt, gt_box_gt_mask, pred_box_pred_mask), PNG, imagenet deprocess.  Each process walks",
        "3 batches of its own form first, then the timed pass of 16 batches, ended by a device synchronise (split: after the",
        "writer's close).  img/s = %d / wall-clock seconds of the timed pass.  Writing the folder took %.1f s (not timed above)."
        % (N, folder_s),
        "",
        "device  (a) the two generate calls and the gt deprocess; nothing copied or written",
        "serial  (b) the same, then .cpu() and Image.save per picture in the loop's thread (the parent commit's way)",
        "split   (c) split.generate_split, %d writer threads" % a.num_writers,
        "",
        "round   device img/s   serial img/s   split img/s   (replayed / eager generate calls of the timed pass: %s)"
        % ", ".join("%s %d / %d" % (m, rounds[-1][m]["replays"], rounds[-1][m]["eager_calls"]) for m in forms),
    ]
    for r, row in enumerate(rounds):
        lines.append("%-7d %-14.1f %-14.1f %-14.1f" % (r + 1, row["device"]["img_per_s"], row["serial"]["img_per_s"],
                                                      row["split"]["img_per_s"]))
    lines += [
        "",
        "median  %-14.1f %-14.1f %-14.1f" % (med["device"], med["serial"], med["split"]),
        "spread  %-14.1f %-14.1f %-14.1f (max - min over the rounds)" % tuple(spread(rate[m]) for m in forms),
        "",
        "split against serial: %.2fx (medians); split is ahead by %.1f img/s, serial's own spread is %.1f img/s."
        % (med["split"] / med["serial"], med["split"] - med["serial"], spread(rate["serial"])),
        "split against device: %.1f%% of the device-only rate." % (100.0 * med["split"] / med["device"]),
        "pictures of serial and split (last round): %d files compared, %d differ." % (n, bad),
        "launches of the package's own kernels in one batch's device work, walked eagerly (torch's own launches — the",
        "encoder's small tensor ops, copies — are not counted): %d; per kernel: %s"
        % (count["launches"], ", ".join("%s %d" % kv for kv in sorted(count["per_kernel"].items()))),
        "",
    ]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.report:
        os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
        with open(a.report, "w") as f:
            f.write(text)
    if bad:
        raise SystemExit("split_speed: %d of %d pictures differ between the serial form and generate_split" % (bad, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["folder", "device", "serial", "split", "count", "same", "all"])
    ap.add_argument("dir")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--out", default=None)
    ap.add_argument("--num_writers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--report", default=None)
    a = ap.parse_args()
    if a.mode == "folder":
        print("folder: %d pictures in %s" % (N, write_folder(a.dir)))
    elif a.mode == "same":
        n, bad = same_pictures(a.dir, a.other)
        print("%d files compared, %d differ" % (n, bad))
        sys.exit(1 if bad else 0)
    elif a.mode == "all":
        run_all(a)
    elif a.mode == "count":
        count_launches(a)
    else:
        one_form(a)


if __name__ == "__main__":
    main()
