"""COCO segmentation masks on the device: the two halves of a batch with `--coco_segmentations` 1 and 0, on one generated folder.

    python tools/coco_masks_bench.py --host                 [--dataset coco|packed_coco] [--batch 16] [--objects 8]
    python tools/coco_masks_bench.py [--mask_size 32|64|0]  [--dataset ...] [--batches 60] [--warmup 10] [--launches]

The folder is tools/input_stage_speed.py's 640 x 480 JPEGs with `--objects` boxes each; this tool adds seeded segmentations
to its annotation files: every instance a polygon of 20 to 200 vertices inside its box, every stuff object a compressed
run-length string of a thresholded noise field inside its box (COCO-Stuff's masks are such strings of thousands of
characters; the lengths made are printed).  No real COCO folder was available where this was written.

`--host` (needs no GPU): BatchBuilder.rows() per batch — the JSON-to-array packing, `round` and, with the switch on, the
strings' decode in the builder's worker threads — in ms per batch, switch on and off.
Without `--host`: the DEVICE half as tools/batch_device_half.py times it — the host half is started and waited for, then two
events bracket finish() — with the switch on at `--mask_size` (0: centres alone, at the dataset's working size) and with the
switch off on the same batches, in one process, the two alternating batch by batch; medians and p10 / p90 over `--batches`
batches after `--warmup`.  `--launches` adds the library's launch counts of one more batch with the switch on.
One JSON line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from input_stage_speed import make_folder  # noqa: E402  (inserts this checkout's root into sys.path)


def counts_to_string(counts):
    """pycocotools' rleToString."""
    out = bytearray()
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            out.append((ch | (0x20 if more else 0)) + 48)
    return out.decode("ascii")


def add_segmentations(root, h=480, w=640):
    """Seeded segmentations for every annotation of make_folder's two files -> (vertices per polygon, characters per string)."""
    from PIL import Image
    rng = np.random.default_rng(7)
    verts, chars = [], []
    for name, stuff in (("instances.json", False), ("stuff.json", True)):
        path = os.path.join(root, name)
        with open(path) as f:
            data = json.load(f)
        for a in data["annotations"]:
            x, y, bw, bh = a["bbox"]
            if not stuff:
                k = int(rng.integers(20, 201))
                ang = np.sort(rng.uniform(0, 2 * np.pi, k))
                rad = rng.uniform(0.55, 1.0, k)
                px = x + bw / 2 + rad * np.cos(ang) * bw / 2
                py = y + bh / 2 + rad * np.sin(ang) * bh / 2
                a["segmentation"] = [[round(float(v), 2) for v in np.stack([px, py], 1).reshape(-1)]]
                verts.append(k)
            else:
                cell = int(rng.choice([6, 8, 12]))
                low = rng.integers(0, 256, size=(h // cell + 1, w // cell + 1), dtype=np.uint8)
                field = np.asarray(Image.fromarray(low, "L").resize((w, h), Image.BICUBIC))
                mask = np.zeros((h, w), bool)
                x0, y0, x1, y1 = int(x), int(y), int(x + bw), int(y + bh)
                mask[y0:y1, x0:x1] = field[y0:y1, x0:x1] > 128
                flat = mask.T.reshape(-1)
                edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
                counts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
                if flat[0]:
                    counts = [0] + counts
                a["segmentation"] = {"size": [h, w], "counts": counts_to_string(counts)}
                chars.append(len(a["segmentation"]["counts"]))
        with open(path, "w") as f:
            json.dump(data, f)
    return verts, chars


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "p10_ms": round(ms[len(ms) // 10], 4),
            "p90_ms": round(ms[len(ms) * 9 // 10], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", choices=["coco", "packed_coco"], default="coco")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--mask_size", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    import torch
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    tmp = tempfile.mkdtemp(prefix="coco_masks_")
    try:
        make_folder(tmp, 2 * a.batch, objects=a.objects)
        verts, chars = add_segmentations(tmp)
        flags = ["--dataset", a.dataset, "--image_size", "%d,%d" % (a.size, a.size), "--batch_size", str(a.batch),
                 "--coco_train_image_dir", os.path.join(tmp, "images"), "--coco_train_instances_json",
                 os.path.join(tmp, "instances.json"), "--coco_train_stuff_json", os.path.join(tmp, "stuff.json"),
                 "--min_objects", "1", "--max_objects", str(a.objects), "--loader_num_workers", str(a.workers), "--no_vgg_loss"]
        dev = torch.device("cuda:0") if not a.host else torch.device("cpu")
        builders = {}
        for on in (1, 0):
            f = flags + ["--coco_segmentations", str(on), "--mask_size", str(a.mask_size if on else 0)]
            ds = folder_dataset(build_parser().parse_args(f), "train")
            assert ds is not None and len(ds) == 2 * a.batch, "the generated folder was not read whole"
            builders[on] = folder_builder(ds, T.make_opt(ds.vocab, f), None, dev)
        lists = [list(range(a.batch)), list(range(a.batch, 2 * a.batch))]
        out = {"dataset": a.dataset, "batch": a.batch, "objects": a.objects, "polygon_vertices": [min(verts), max(verts)],
               "string_characters": [min(chars), int(statistics.median(chars)), max(chars)], "workers": a.workers}
        if a.host:
            sizes = np.tile(np.asarray([[480, 640]], np.int64), (a.batch, 1))
            ms = {1: [], 0: []}
            for k in range(a.warmup + a.batches):
                for on in (1, 0):
                    b = builders[on]
                    t0 = time.perf_counter()
                    b.rows(lists[k % 2], sizes, b.draw(lists[k % 2]))
                    if k >= a.warmup:
                        ms[on].append(1e3 * (time.perf_counter() - t0))
            out.update({"half": "host: rows() per batch", "switch_on": spread(ms[1]), "switch_off": spread(ms[0])})
        else:
            assert torch.cuda.is_available(), "the device half needs the GPU"
            ms, shape = {1: [], 0: []}, None
            for k in range(a.warmup + a.batches):
                for on in (1, 0):
                    b = builders[on]
                    pending = b.start(lists[k % 2])
                    for fut in pending.futures:
                        fut.result()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    batch = b.finish(pending)
                    e1.record()
                    e1.synchronize()
                    if k >= a.warmup:
                        ms[on].append(e0.elapsed_time(e1))
                    if on:
                        shape = [list(batch[1].shape), list(batch[3].shape), None if batch[6] is None else list(batch[6].shape)]
            out.update({"half": "device: finish() per batch", "mask_size": a.mask_size, "objs_triplets_masks": shape,
                        "switch_on": spread(ms[1]), "switch_off": spread(ms[0])})
            if a.launches:
                from canonicalsg2im_amd import _lib
                pending = builders[1].start(lists[0])
                _lib.prof_enable(1)
                _lib.prof_reset()
                builders[1].finish(pending)
                torch.cuda.synchronize()
                read = _lib.prof_read()
                out["entries"] = {k: v[1] for k, v in read.items()}
                out["coco_masks_kernel_ms"] = round(read["coco_masks"][0], 4)
                _lib.prof_enable(0)
        for b in builders.values():
            b.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
