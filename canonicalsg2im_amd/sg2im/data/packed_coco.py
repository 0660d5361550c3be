"""COCO / COCO-Stuff from a folder of pictures, with the input stage on the device (reference: sg2im/data/packed_coco.py).

`PackedCocoSceneGraphDataset` reads the two annotation files and applies the reference's rules (:151-265): an image must
appear in the stuff annotations; an object stays when its box covers more than `min_object_size` of the image, its category
is whitelisted and it is not "other" (unless `include_other`); `__image__` is object 0; an image stays when
min_objects <= its objects <= max_objects; `max_samples` caps the length.  The vocabulary has the reference's keys.

What the host does per image is: open the file, convert('RGB'), copy the bytes into a pinned staging buffer, divide the
boxes by the decoded size.  Everything else of the reference's `__getitem__` and collate runs on the device
(`CocoBatchBuilder`): Pillow's resize, ToTensor and Normalize in `ops.preprocess_images` (bit for bit), the `__image__`
row, the canonical graph and the padding in `collate.packed_batch`.

MASKS ARE NOT SUPPORTED: decoding COCO's polygon / RLE segmentations needs pycocotools, which this package does not depend
on, so `mask_size` must be 0.  Object centres are therefore BOX centres.  The reference takes the centroid of the decoded
mask for the location relations even with mask_size == 0 (:336-351), so for concave objects whose mask centroid and box
centre fall on different sides of another object's the graphs can differ from the reference's."""
import json
import os
from collections import defaultdict

import numpy as np
import torch

from . import register_augmented_relations
from .collate import packed_batch
from .loader import MAX_LOADER_THREADS, BatchBuilder, _Pending, _Staging, epoch_batches  # noqa: F401  (their first home)

_NO_MASKS = ("PackedCocoSceneGraphDataset: mask_size must be 0 (got %d): segmentation masks need pycocotools, which is not "
             "a dependency; object centres are box centres, not mask centroids as in the reference")


class PackedCocoSceneGraphDataset:
    def __init__(self, image_dir, instances_json, stuff_json, image_size=(64, 64), mask_size=0, normalize_images=True,
                 max_samples=None, min_object_size=0.02, min_objects=16, max_objects=1000, include_other=False,
                 instance_whitelist=None, stuff_whitelist=None):
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)
        self.image_dir = image_dir
        self.image_size = tuple(image_size)
        self.normalize_images = bool(normalize_images)
        self.max_samples = max_samples
        with open(instances_json, "r") as f:
            instances = json.load(f)
        with open(stuff_json, "r") as f:
            stuff = json.load(f)

        self.image_id_to_filename, self.image_id_to_size = {}, {}
        image_ids = []
        for im in instances["images"]:
            image_ids.append(im["id"])
            self.image_id_to_filename[im["id"]] = im["file_name"]
            self.image_id_to_size[im["id"]] = (im["width"], im["height"])

        name_to_idx, idx_to_name = {}, {}
        names = {"instances": [], "stuff": []}
        for kind, data in (("instances", instances), ("stuff", stuff)):
            for cat in data["categories"]:
                names[kind].append(cat["name"])
                idx_to_name[cat["id"]] = cat["name"]
                name_to_idx[cat["name"]] = cat["id"]
        whitelist = set(names["instances"] if instance_whitelist is None else instance_whitelist) | \
            set(names["stuff"] if stuff_whitelist is None else stuff_whitelist)

        self.image_id_to_objects = defaultdict(list)
        with_stuff = set()
        for kind, data in (("instances", instances), ("stuff", stuff)):
            for obj in data["annotations"]:
                image_id = obj["image_id"]
                if kind == "stuff":
                    with_stuff.add(image_id)
                _, _, w, h = obj["bbox"]
                WW, HH = self.image_id_to_size[image_id]
                name = idx_to_name[obj["category_id"]]
                if (w * h) / (WW * HH) > min_object_size and name in whitelist and (name != "other" or include_other):
                    self.image_id_to_objects[image_id].append(obj)
        for image_id in set(self.image_id_to_filename) - with_stuff:
            self.image_id_to_filename.pop(image_id, None)
            self.image_id_to_size.pop(image_id, None)
            self.image_id_to_objects.pop(image_id, None)
        image_ids = [i for i in image_ids if i in with_stuff]

        name_to_idx["__image__"] = 0                        # COCO's category ids start at 1
        if len(name_to_idx) != len(set(name_to_idx.values())):
            raise ValueError("two categories share an id")
        names_by_idx = ["NONE"] * (1 + max(name_to_idx.values()))
        for name, idx in name_to_idx.items():
            names_by_idx[idx] = name
        self.image_ids = [i for i in image_ids if min_objects <= len(self.image_id_to_objects[i]) <= max_objects]

        self.vocab = {"object_name_to_idx": name_to_idx, "pred_name_to_idx": {}, "object_idx_to_name": names_by_idx}
        register_augmented_relations(self.vocab)
        self.vocab["attributes"] = {"objects": name_to_idx}
        self.vocab["reverse_attributes"] = {"objects": {v: k for k, v in name_to_idx.items()}}

    def __len__(self):
        return len(self.image_ids) if self.max_samples is None else min(len(self.image_ids), self.max_samples)

    def open(self, index):
        """The opened picture (header read, pixels not yet decoded) of sample `index`."""
        from PIL import Image                  # only here: importing the package never needs PIL
        return Image.open(os.path.join(self.image_dir, self.image_id_to_filename[self.image_ids[index]]))

    def annotations(self, index, WW, HH):
        """(objs int64 (n,), boxes fp32 (n,4) = x/WW, y/HH, w/WW, h/HH) of sample `index` for a picture decoded at WW x HH."""
        rows = self.image_id_to_objects[self.image_ids[index]]
        objs = np.asarray([o["category_id"] for o in rows], np.int64)
        boxes = np.asarray([[o["bbox"][0] / WW, o["bbox"][1] / HH, o["bbox"][2] / WW, o["bbox"][3] / HH] for o in rows],
                           np.float64).reshape(-1, 4).astype(np.float32)
        return objs, boxes

    def load(self, index):
        """One sample on the host: (pixels uint8 (h,w,3), objs (n,), boxes (n,4), image id)."""
        with self.open(index) as im:
            WW, HH = im.size
            pixels = np.asarray(im.convert("RGB"))
        objs, boxes = self.annotations(index, WW, HH)
        return pixels, torch.from_numpy(objs), torch.from_numpy(boxes), self.image_ids[index]


class CocoBatchBuilder(BatchBuilder):
    """Batches of a PackedCocoSceneGraphDataset as the 8-tuple Trainer.step takes (loader.BatchBuilder has the staging, the
    look-ahead and the rule that the workers make no HIP call).

    start(indices): `num_workers` threads open the files and decode them into a pinned buffer; descriptor, image ids,
    objects and boxes are laid out in a second one.  finish(pending), on the current stream: ONE copy of the packed bytes
    and ONE of the second buffer to the device, ops.preprocess_images, collate.packed_batch."""

    @staticmethod
    def _decode(im, dst):
        try:
            dst[:] = np.asarray(im.convert("RGB")).reshape(-1)
        finally:
            im.close()

    def start(self, indices):
        """The host half.  Called by the consumer's thread between two steps: the one HIP call it can make, the pinned
        allocation when a staging buffer has to grow, is made here and not by a worker."""
        B = len(indices)
        slot = self._take_slot()
        opened = list(self.pool.map(self.ds.open, indices))              # headers: the sizes
        sizes = [(im.size[1], im.size[0]) for im in opened]              # (h, w)
        ann = [self.ds.annotations(i, w, h) for i, (h, w) in zip(indices, sizes)]
        O = max(a[0].shape[0] for a in ann)
        offsets = np.concatenate([[0], np.cumsum([3 * h * w for h, w in sizes])]).astype(np.int64)
        stage = self.pixels[slot].take(int(offsets[-1]))[:int(offsets[-1])]
        host = stage.numpy()                                              # the workers write through numpy: no torch call
        futures = [self.pool.submit(self._decode, im, host[offsets[i]:offsets[i + 1]]) for i, im in enumerate(opened)]
        # descriptor | image ids | objects (int64), then boxes (fp32): one buffer, one copy
        n64 = 3 * B + B + B * O
        meta = self.meta[slot].take(8 * n64 + 16 * B * O)[:8 * n64 + 16 * B * O]
        i64 = meta[:8 * n64].view(torch.int64)
        f32 = meta[8 * n64:].view(torch.float32).view(B, O, 4)
        desc_host = i64[:3 * B].view(B, 3)
        desc_host[:, 0] = torch.from_numpy(offsets[:-1])
        desc_host[:, 1:] = torch.as_tensor(sizes, dtype=torch.int64)
        i64[3 * B:4 * B] = torch.as_tensor([self.ds.image_ids[i] for i in indices], dtype=torch.int64)
        objs_host = i64[4 * B:].view(B, O)
        objs_host.zero_()
        f32.fill_(-1.0)
        for b, (o, bx) in enumerate(ann):
            objs_host[b, :o.shape[0]] = torch.from_numpy(o)
            f32[b, :bx.shape[0]] = torch.from_numpy(bx)
        return _Pending(futures=futures, slot=slot, stage=stage, meta=meta, desc=desc_host.clone(), B=B, O=O, n64=n64)

    def finish(self, p):
        """The device half, enqueued on the current stream."""
        from ... import ops
        B, O, n64 = p.B, p.O, p.n64
        src, meta_dev = self._upload(p)
        i64_dev = meta_dev[:8 * n64].view(torch.int64)
        H, W = self.ds.image_size
        imgs = ops.preprocess_images(src, i64_dev[:3 * B].view(B, 3), H, W, normalize=self.ds.normalize_images,
                                     desc_host=p.desc)
        raw = [imgs, i64_dev[4 * B:].view(B, O, 1), meta_dev[8 * n64:].view(torch.float32).view(B, O, 4), None, None, None,
               None, i64_dev[3 * B:4 * B]]
        return packed_batch(self.args, self.trainer, raw, self.dev)


def build_coco_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory does not
    exist.  Paths: --coco_<split>_image_dir / _instances_json / _stuff_json, by default the reference's layout under
    --dataroot (sg2im/data/dataset_params.py:75-84)."""
    root = os.path.join(args.dataroot, "MSCoco")
    image_dir = getattr(args, "coco_%s_image_dir" % split) or os.path.join(root, "images", "%s2017" % split)
    if not os.path.isdir(image_dir):
        return None
    if args.mask_size:
        raise NotImplementedError(_NO_MASKS % args.mask_size)
    inst = getattr(args, "coco_%s_instances_json" % split) or os.path.join(root, "annotations", "instances_%s2017.json" % split)
    stuff = getattr(args, "coco_%s_stuff_json" % split) or os.path.join(root, "annotations", "stuff_%s2017.json" % split)
    return PackedCocoSceneGraphDataset(
        image_dir, inst, stuff, image_size=args.image_size, mask_size=args.mask_size,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        min_object_size=args.min_object_size, min_objects=args.min_objects or 16, max_objects=args.max_objects or 1000)
