"""The input stage alone: the reference-style host pipeline against the device one, per batch, on generated pictures.

    python tools/input_stage_speed.py --mode host|device [--batch 16] [--size 256] [--workers 16] [--calls 20] [--warmup 5]
                                      [--dataset packed_coco|packed_clevr|packed_vg]
    python tools/input_stage_speed.py --make-folder DIR [--images 64]       (also writes the two annotation files)

host   = what the reference's loader does per sample (sg2im/data/packed_coco.py:294-301): PIL open, convert('RGB'),
         Resize (Pillow's bilinear), ToTensor (.float().div(255)), Normalize (.sub(mean).div(std)) in `--workers` threads,
         torch.cat of the batch, then ONE fp32 host-to-device copy from pinned memory.
device = PIL open, convert('RGB'), byte copy into pinned memory in `--workers` threads, ONE uint8 host-to-device copy,
         ops.preprocess_images.
Both end in a device synchronise; a call is one batch.  One process measures one mode: run the two alternately, in fresh
processes, and compare medians.  The pictures are 480 x 640 JPEGs of seeded smooth noise (decode cost near a
photograph's), generated into a temporary folder that is removed at exit.

--dataset (default packed_coco: the above) chooses the pictures and the constants of the dataset's input stage:
packed_clevr = 320 x 480 RGBA PNGs, Normalize(0.5, 0.5), and in device mode the decoded RGBA bytes go up as 4-byte pixels
(no convert('RGB') on the host; descriptor rows of four columns); packed_vg = the JPEGs, Normalize(0.5, 0.5).  The object
rows and boxes (ops.clevr_boxes, ops.vg_rows: one small launch per batch) are not part of either mode.  Neither of the two
new modes has been run on a device yet: no number is claimed from them."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# dataset -> (mean, std, picture h, w, mode the pictures are saved in)
DATASETS = {"packed_coco": (MEAN, STD, 480, 640, "RGB"), "packed_clevr": ((0.5,) * 3, (0.5,) * 3, 320, 480, "RGBA"),
            "packed_vg": ((0.5,) * 3, (0.5,) * 3, 480, 640, "RGB")}


def make_folder(root, n, h=480, w=640, objects=16, mode="RGB"):
    """n seeded JPEGs (mode RGBA: PNGs with a seeded alpha byte) under root/images plus instances.json / stuff.json with
    `objects` boxes per picture."""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    rng = np.random.default_rng(0)
    images, things, stuff = [], [], []
    for i in range(n):
        low = rng.integers(0, 256, size=(h // 8, w // 8, 3), dtype=np.uint8)
        px = np.asarray(Image.fromarray(low, "RGB").resize((w, h), Image.BICUBIC)).astype(np.int16)
        px = np.clip(px + rng.integers(-12, 13, size=px.shape), 0, 255).astype(np.uint8)
        if mode == "RGBA":
            name = "%06d.png" % i
            px = np.concatenate([px, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], 2)
            Image.fromarray(px, "RGBA").save(os.path.join(root, "images", name))
        else:
            name = "%06d.jpg" % i
            Image.fromarray(px, "RGB").save(os.path.join(root, "images", name), quality=90)
        images.append({"id": i + 1, "file_name": name, "width": w, "height": h})
        for k in range(objects):
            bw, bh = rng.uniform(0.2, 0.5, size=2)
            x, y = rng.uniform(0, 1 - bw), rng.uniform(0, 1 - bh)
            ann = {"id": len(things) + len(stuff) + 1, "image_id": i + 1, "category_id": 1 + k % 80 if k % 4 else 92 + k % 90,
                   "bbox": [x * w, y * h, bw * w, bh * h]}
            (things if k % 4 else stuff).append(ann)
    cats_t = [{"id": c, "name": "thing_%d" % c} for c in range(1, 81)]
    cats_s = [{"id": c, "name": "stuff_%d" % c} for c in range(92, 183)]
    with open(os.path.join(root, "instances.json"), "w") as f:
        json.dump({"images": images, "categories": cats_t, "annotations": things}, f)
    with open(os.path.join(root, "stuff.json"), "w") as f:
        json.dump({"images": images, "categories": cats_s, "annotations": stuff}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["host", "device"])
    ap.add_argument("--make-folder")
    ap.add_argument("--dataset", choices=sorted(DATASETS), default="packed_coco")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    h, w, mode = DATASETS[a.dataset][2:]
    if a.make_folder:
        make_folder(a.make_folder, a.images, h, w, mode=mode)
        return
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="input_stage_")
    try:
        make_folder(tmp, a.images, h, w, mode=mode)
        measure(a, tmp, dev)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure(a, tmp, dev):
    from PIL import Image
    files = sorted(os.path.join(tmp, "images", f) for f in os.listdir(os.path.join(tmp, "images")))
    pool = ThreadPoolExecutor(max_workers=min(a.workers, 16))
    H = W = a.size
    mean3, std3 = DATASETS[a.dataset][:2]
    mean = torch.as_tensor(mean3, dtype=torch.float32).view(3, 1, 1)
    std = torch.as_tensor(std3, dtype=torch.float32).view(3, 1, 1)
    px = a.dataset == "packed_clevr"                   # device mode: pictures go up in their decoded mode, 3 or 4 bytes a pixel

    if a.mode == "host":
        pinned = torch.empty((a.batch, 3, H, W), dtype=torch.float32, pin_memory=True)

        def one(job):
            slot, path = job
            with Image.open(path) as im:
                u8 = np.asarray(im.convert("RGB").resize((W, H), Image.BILINEAR))
            t = torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().float().div(255)
            pinned[slot] = t.sub_(mean).div_(std)

        def call(paths):
            list(pool.map(one, list(enumerate(paths))))
            out = pinned.to(dev, non_blocking=True)
            torch.cuda.synchronize()
            return out
    else:
        from canonicalsg2im_amd import ops
        largest = 0                                     # bytes of the largest picture, from the files' headers
        for path in files:
            with Image.open(path) as im:
                largest = max(largest, (4 if px else 3) * im.size[0] * im.size[1])
        staging = torch.empty(a.batch * (largest + 4), dtype=torch.uint8, pin_memory=True)

        def call(paths):
            opened = list(pool.map(Image.open, paths))
            sizes = [(im.size[1], im.size[0]) for im in opened]
            modes = ["RGBA" if px and im.mode == "RGBA" else "RGB" for im in opened]
            nbytes = [len(m) * h * w for m, (h, w) in zip(modes, sizes)]
            step = [-(-n // 4) * 4 for n in nbytes] if px else nbytes       # 4-byte pixels start on a 4-byte boundary
            off = np.concatenate([[0], np.cumsum(step)]).astype(np.int64)

            def decode(i):
                im = opened[i] if opened[i].mode == modes[i] else opened[i].convert(modes[i])
                staging[off[i]:off[i] + nbytes[i]].numpy()[:] = np.asarray(im).reshape(-1)
                opened[i].close()

            list(pool.map(decode, range(len(paths))))
            desc = torch.as_tensor([[off[i], h, w] + ([len(modes[i])] if px else []) for i, (h, w) in enumerate(sizes)],
                                   dtype=torch.int64)
            out = ops.preprocess_images(staging[:off[-1]].to(dev, non_blocking=True), desc, H, W, mean=mean3, std=std3)
            torch.cuda.synchronize()
            return out

    times = []
    for k in range(a.warmup + a.calls):
        paths = [files[(k * a.batch + j) % len(files)] for j in range(a.batch)]
        t0 = time.perf_counter()
        call(paths)
        if k >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"mode": a.mode, "dataset": a.dataset, "batch": a.batch, "size": a.size, "workers": min(a.workers, 16), "calls": a.calls,
                      "median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3),
                      "max_ms": round(max(times), 3)}), flush=True)
    pool.shutdown()


if __name__ == "__main__":
    main()
