"""The DEVICE half of a folder dataset's batch, timed with events: what BatchBuilder.finish enqueues and waits for.

    python tools/batch_device_half.py --dataset coco|packed_coco|vg|packed_vg|clevr|packed_clevr [--package-root DIR]
                                      [--batch 16] [--size 256] [--objects 8] [--batches 60] [--warmup 10]
                                      [--learned_transitivity 0|1] [--use_transitivity 0|1] [--launches]

A batch's host half (PIL decode into pinned memory, the draws, the second staging buffer) is started and WAITED FOR first;
then two events bracket finish(): the two uploads, the dataset's kernels, ops.preprocess_images, the `__image__` row and the
canonical graph with its one read-back of the triplet counts.  So the figure is device time plus the host time between the
launches of one batch, per batch; the median and the spread over `--batches` batches after `--warmup` are printed as one
JSON line.  The pictures are tools/input_stage_speed.py's 480 x 640 JPEGs with `--objects` boxes each, generated into a
temporary folder that is removed at exit.

`--dataset vg` and `--dataset packed_vg` read the same pictures with a seeded split file beside them: `--objects` objects per
picture, all of them kept (max_objects = `--objects`), and as many annotated relationships among the vocabulary's plain
predicates; each gets the vocab.json its dataset expects (with and without the location predicates).  `--launches` adds the
library's launch counts of one more batch, per kernel name.

`--dataset clevr` and `--dataset packed_clevr` read a CLEVR folder of their own: 480 x 320 RGBA renders of seeded bytes and a
scenes file with `--objects` objects per scene (10 is CLEVR's most), whose four relationships are four seeded total orders.

`--package-root DIR` imports canonicalsg2im_amd from another checkout (built there), so that two commits are timed by one
tool: run them alternately, in fresh processes.  It uses nothing a checkout before the `coco` dataset lacks, for
`--dataset packed_coco`."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from input_stage_speed import make_folder  # noqa: E402  (inserts this checkout's root into sys.path)


def make_vg_tables(root, n, objects, unpacked):
    """train.npz and vocab.json beside make_folder's pictures: `objects` objects per picture with boxes inside the 480 x 640
    frame and `objects` relationships between two different ones.  unpacked: vocab.json without the location predicates."""
    import numpy as np
    from canonicalsg2im_amd.synth import make_vocab
    v = make_vocab("vg")
    plain = [p for p in v["pred_idx_to_name"] if not p.startswith("__")]
    preds = ["__in_image__"] + plain if unpacked else list(v["pred_idx_to_name"])
    vocab = {"object_name_to_idx": v["object_name_to_idx"], "object_idx_to_name": v["object_idx_to_name"],
             "pred_name_to_idx": {p: i for i, p in enumerate(preds)}, "pred_idx_to_name": preds}
    with open(os.path.join(root, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    rng = np.random.default_rng(1)
    names = rng.integers(1, len(v["object_idx_to_name"]), size=(n, objects)).astype(np.int32)
    wh = rng.integers(60, 300, size=(n, objects, 2))
    xy = (rng.random((n, objects, 2)) * (np.asarray([640, 480]) - wh)).astype(np.int64)
    subjects = rng.integers(0, objects, size=(n, objects))
    others = (subjects + rng.integers(1, objects, size=(n, objects))) % objects
    which = rng.integers(0, len(plain), size=(n, objects))
    ids = np.asarray([vocab["pred_name_to_idx"][p] for p in plain])
    np.savez(os.path.join(root, "train.npz"), image_paths=np.asarray(["%06d.jpg" % i for i in range(n)]),
             object_names=names, object_boxes=np.concatenate([xy, wh], 2).astype(np.int32),
             objects_per_image=np.full(n, objects, np.int32), relationship_subjects=subjects.astype(np.int32),
             relationship_predicates=ids[which].astype(np.int32), relationship_objects=others.astype(np.int32),
             relationships_per_image=np.full(n, objects, np.int32))


def make_clevr_folder(root, n, objects):
    """<root>/CLEVR/CLEVR_Dialog in the reference's layout: n RGBA renders of 480 x 320 under images/train/ and
    scenes/CLEVR_train_scenes.json, `objects` objects per scene, every relationship a total order."""
    import numpy as np
    from PIL import Image
    base = os.path.join(root, "CLEVR", "CLEVR_Dialog")
    os.makedirs(os.path.join(base, "scenes"))
    os.makedirs(os.path.join(base, "images", "train"))
    rng = np.random.default_rng(2)
    shapes, colors = ["cube", "sphere", "cylinder"], ["gray", "red", "blue", "green", "brown", "purple", "cyan", "yellow"]
    scenes = []
    for i in range(n):
        name = "CLEVR_train_%06d.png" % i
        Image.fromarray(rng.integers(0, 256, size=(320, 480, 4), dtype=np.uint8), "RGBA").save(
            os.path.join(base, "images", "train", name))
        theta = float(rng.uniform(-0.6, 0.6))
        objs = [{"shape": shapes[(i + o) % 3], "color": colors[(i + o) % 8], "material": ["rubber", "metal"][o % 2],
                 "size": ["small", "large"][o % 2], "3d_coords": [float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), [0.35, 0.7][o % 2]],
                 "pixel_coords": [int(rng.integers(20, 460)), int(rng.integers(20, 300)), float(rng.uniform(7, 14))]}
                for o in range(objects)]
        rel = {}
        for key in ("right", "behind", "front", "left"):
            rank = rng.permutation(objects)
            rel[key] = [[int(o2) for o2 in range(objects) if rank[o2] > rank[o1]] for o1 in range(objects)]
        scenes.append({"image_index": i, "image_filename": name, "split": "train", "objects": objs, "relationships": rel,
                       "directions": {"right": [float(np.cos(theta)), float(np.sin(theta)), 0.0]}})
    with open(os.path.join(base, "scenes", "CLEVR_train_scenes.json"), "w") as f:
        json.dump({"scenes": scenes}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", choices=["coco", "packed_coco", "vg", "packed_vg", "clevr", "packed_clevr"], default="coco")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--package-root")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--learned_transitivity", type=int, default=0)
    ap.add_argument("--use_transitivity", type=int, default=0)
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="device_half_")
    try:
        clevr = a.dataset in ("clevr", "packed_clevr")
        if clevr:
            make_clevr_folder(tmp, 2 * a.batch, a.objects)
        else:
            make_folder(tmp, 2 * a.batch, objects=a.objects)
        flags = ["--dataset", a.dataset, "--image_size", "%d,%d" % (a.size, a.size), "--batch_size", str(a.batch),
                 "--dataroot", tmp, "--loader_num_workers", str(a.workers),
                 "--learned_transitivity", str(a.learned_transitivity), "--use_transitivity", str(a.use_transitivity)] if clevr else ["--dataset", a.dataset, "--image_size", "%d,%d" % (a.size, a.size), "--batch_size", str(a.batch),
                 "--coco_train_image_dir", os.path.join(tmp, "images"), "--coco_train_instances_json",
                 os.path.join(tmp, "instances.json"), "--coco_train_stuff_json", os.path.join(tmp, "stuff.json"),
                 "--min_objects", "1", "--max_objects", str(a.objects), "--loader_num_workers", str(a.workers),
                 "--learned_transitivity", str(a.learned_transitivity)]
        if a.dataset in ("vg", "packed_vg"):
            make_vg_tables(tmp, 2 * a.batch, a.objects, a.dataset == "vg")
            flags += ["--vg_image_dir", os.path.join(tmp, "images"), "--train_h5", os.path.join(tmp, "train.npz"),
                      "--vocab_json", os.path.join(tmp, "vocab.json")]
        ds = folder_dataset(build_parser().parse_args(flags), "train")
        assert ds is not None and len(ds) == 2 * a.batch, "the generated folder was not read whole"
        opt = T.make_opt(ds.vocab, flags + ["--no_vgg_loss"])
        builder = folder_builder(ds, opt, None, dev)
        lists = [list(range(a.batch)), list(range(a.batch, 2 * a.batch))]
        ms, shape = [], None
        for k in range(a.warmup + a.batches):
            pending = builder.start(lists[k % 2])
            for f in pending.futures:
                f.result()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            batch = builder.finish(pending)
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
            shape = [list(batch[0].shape), list(batch[1].shape), list(batch[3].shape)]
        launches = None
        if a.launches:
            from canonicalsg2im_amd import _lib
            pending = builder.start(lists[0])
            _lib.prof_enable(1)
            _lib.prof_reset()
            builder.finish(pending)
            torch.cuda.synchronize()
            launches = {k: v[1] for k, v in _lib.prof_read().items()}
            _lib.prof_enable(0)
        builder.close()
        ms.sort()
        print(json.dumps({"dataset": a.dataset, "package": a.package_root or ".", "objects": a.objects, "entries": launches,
                          "batches": len(ms), "imgs_objs_triplets": shape, "learned_transitivity": a.learned_transitivity,
                          "use_transitivity": a.use_transitivity,
                          "median_ms": round(statistics.median(ms), 4), "p10_ms": round(ms[len(ms) // 10], 4),
                          "p90_ms": round(ms[len(ms) * 9 // 10], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
