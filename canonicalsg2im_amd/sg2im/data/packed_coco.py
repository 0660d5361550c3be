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
from .loader import BatchBuilder

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
    """Batches of a PackedCocoSceneGraphDataset (loader.BatchBuilder has the two halves of a batch): every picture goes up as
    RGB; the fields of its own are the category ids and the boxes over the decoded sizes, and no kernel of its own runs."""

    def rows(self, indices, sizes, drawn):
        ann = [self.ds.annotations(i, w, h) for i, (h, w) in zip(indices, sizes.tolist())]
        O = max(a[0].shape[0] for a in ann)
        objs = np.zeros((len(ann), O, 1), np.int64)
        boxes = np.full((len(ann), O, 4), -1.0, np.float32)
        for b, (o, bx) in enumerate(ann):
            objs[b, :o.shape[0], 0] = o
            boxes[b, :bx.shape[0]] = bx
        return {"objs": objs, "boxes": boxes}, {}

    def assemble(self, dev, p):
        return dev["objs"], dev["boxes"], None, None


PackedCocoSceneGraphDataset.builder_class = CocoBatchBuilder


def split_image_dir(args, split):
    """Where the split's pictures are looked for: --coco_<split>_image_dir, else the reference's layout under --dataroot."""
    return getattr(args, "coco_%s_image_dir" % split) or os.path.join(args.dataroot, "MSCoco", "images", "%s2017" % split)


def build_coco_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory does not
    exist.  Paths: --coco_<split>_image_dir / _instances_json / _stuff_json, by default the reference's layout under
    --dataroot (sg2im/data/dataset_params.py:75-84)."""
    root = os.path.join(args.dataroot, "MSCoco")
    image_dir = split_image_dir(args, split)
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
