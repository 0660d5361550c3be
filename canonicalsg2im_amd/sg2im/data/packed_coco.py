"""COCO / COCO-Stuff from a folder of pictures, with the input stage on the device (reference: sg2im/data/packed_coco.py).

`PackedCocoSceneGraphDataset` reads the two annotation files and applies the reference's rules (:151-265): an image must
appear in the stuff annotations; an object stays when its box covers more than `min_object_size` of the image, its category
is whitelisted and it is not "other" (unless `include_other`); `__image__` is object 0; an image stays when
min_objects <= its objects <= max_objects; `max_samples` caps the length.  The vocabulary has the reference's keys.

What the host does per image is: open the file, convert('RGB'), copy the bytes into a pinned staging buffer, divide the
boxes by the decoded size.  Everything else of the reference's `__getitem__` and collate runs on the device
(`CocoBatchBuilder`): Pillow's resize, ToTensor and Normalize in `ops.preprocess_images` (bit for bit), the `__image__`
row, the canonical graph and the padding in `collate.packed_batch`.

MASKS ARE OPT-IN: `segmentations=True` (`--coco_segmentations 1`).  Without it nothing of an annotation's segmentation is
read, `mask_size` must be 0 and object centres are BOX centres — for concave objects whose mask centroid and box centre fall
on different sides of another object's the graphs then differ from the reference's, which takes the centroid of the decoded
mask for the location relations even with mask_size == 0 (:336-351).

With it, every object's segmentation is decoded on the device (`ops.coco_masks`, csrc/coco_masks.hip): seg_to_mask for
polygon lists, run lists and compressed strings, the crop to the rounded box, the nearest-neighbour resize to M x M and the
mask's centroid as the object's centre.  `mask_size` M may then be any power of two from 2 to 64 and the batch carries
masks (B, O + 1, M, M) with the reference's all-ones `__image__` row; with mask_size == 0 the masks are decoded at the
reference's working size (64 here, :141-143; 32 for `coco`), used for the centres only, and the batch's mask slot stays
None.  The host does what is host work: JSON lists to arrays, Python's `round` for the crop, and the compressed strings'
characters to run lengths (`decode_counts`, vectorised).  The reference does this through pycocotools and OpenCV, which this
package does not depend on; their arithmetic is restated from their public sources (tests/mask_cases.py), and EQUALITY WITH
THEIR OUTPUT HAS NOT BEEN RUN — they are not installed where this was built — which is why the path is opt-in.
Refused when a sample is loaded, with a ValueError naming the image: a run-length segmentation whose `size` is not the
decoded picture's, and a box whose rounded crop is empty (the reference's cv2.resize raises there).  A polygon list without
polygons gives an empty mask and the box centre."""
import json
import os
from collections import defaultdict

import numpy as np
import torch

from . import register_augmented_relations
from .loader import BatchBuilder

_NO_MASKS = ("PackedCocoSceneGraphDataset: mask_size must be 0 (got %d): segmentation masks need pycocotools, which is not "
             "a dependency; object centres are box centres, not mask centroids as in the reference.  --coco_segmentations 1 "
             "(segmentations=True) decodes them on the device instead")
_BAD_MASK_SIZE = "PackedCocoSceneGraphDataset: with segmentations, mask_size must be 0 or a power of two in 2 .. 64 (got %d)"
_BAD_RLE_SIZE = "image %s: object %d has a run-length segmentation of size %s, the decoded picture is %s (HH x WW)"
_EMPTY_CROP = "image %s: object %d with bbox %s has an empty mask crop in the %d x %d picture (WW x HH)"
_BAD_POLYGON = "image %s: object %d has a polygon coordinate beyond +-1e6 pixels, or not finite"
MAX_POLYGON_COORD = 1.0e6                                  # CSG_COCO_MASKS_MAX_COORD


def decode_counts(s):
    """The run lengths of a COCO compressed RLE string (pycocotools' rleFrString) -> int64 array, without a Python loop over
    the characters: five payload bits per character from 48 up, bit 0x20 continues a count, bit 0x10 of a count's last
    character extends its sign, and from the fourth count on a count is a difference to the count two places back."""
    c = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, np.int64)
    last = (c & 0x20) == 0
    if not last[-1]:
        raise ValueError("a compressed RLE string ends inside a count")
    starts = np.concatenate([[0], np.flatnonzero(last)[:-1] + 1])
    k = np.arange(c.size) - np.repeat(starts, np.diff(np.concatenate([starts, [c.size]])))
    if int(k.max()) > 11:
        raise ValueError("a compressed RLE string has a count of more than 12 characters")
    x = np.add.reduceat((c & 0x1f) << (5 * k), starts)      # the payloads do not overlap: a sum is the OR
    ends = np.flatnonzero(last)
    x = x - (((c[ends] & 0x10) != 0).astype(np.int64) << (5 * (k[ends] + 1)))
    out = x.copy()
    out[1::2] = np.cumsum(x[1::2])                          # cnts[m] = x[m] + cnts[m - 2] for m > 2, and cnts[1] = x[1]
    if out.size > 2:
        out[2::2] = np.cumsum(x[2::2])                      # the even chain starts at cnts[2] = x[2]; cnts[0] stands alone
    return out


class PackedCocoSceneGraphDataset:
    default_mask_size = 64                                 # what the reference decodes at with mask_size == 0 (:141-143)

    def __init__(self, image_dir, instances_json, stuff_json, image_size=(64, 64), mask_size=0, normalize_images=True,
                 max_samples=None, min_object_size=0.02, min_objects=16, max_objects=1000, include_other=False,
                 instance_whitelist=None, stuff_whitelist=None, segmentations=False):
        self.segmentations = bool(segmentations)
        if mask_size and not self.segmentations:
            raise NotImplementedError(_NO_MASKS % mask_size)
        if mask_size and (mask_size < 2 or mask_size > 64 or mask_size & (mask_size - 1)):
            raise ValueError(_BAD_MASK_SIZE % mask_size)
        self.mask_size = int(mask_size)
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

    def segmentation_rows(self, index, WW, HH):
        """The segmentations of sample `index` for a picture decoded at WW x HH, one row per object in the order of
        `annotations`: (kind, crop, payload) with kind 1 = polygons, payload a list of fp64 (k,2) vertex arrays, or
        kind 2 = runs, payload the int64 toggles (the running sums of the run lengths); crop = (x0, y0, x1, y1) of
        mask[my0:my1, mx0:mx1] as the reference rounds and a slice clamps it (:317-321)."""
        image_id = self.image_ids[index]
        out = []
        for k, o in enumerate(self.image_id_to_objects[image_id]):
            x, y, w, h = o["bbox"]
            mx0, mx1 = int(round(x)), int(round(x + w))
            my0, my1 = int(round(y)), int(round(y + h))
            x0, x1, _ = slice(mx0, max(mx0 + 1, mx1)).indices(WW)
            y0, y1, _ = slice(my0, max(my0 + 1, my1)).indices(HH)
            if x1 <= x0 or y1 <= y0:
                raise ValueError(_EMPTY_CROP % (image_id, k, list(o["bbox"]), WW, HH))
            seg = o["segmentation"]
            if isinstance(seg, list):
                polys = [np.asarray(p, np.float64).reshape(-1)[:2 * (len(p) // 2)].reshape(-1, 2) for p in seg]
                if any(not bool((np.abs(p) <= MAX_POLYGON_COORD).all()) for p in polys):
                    raise ValueError(_BAD_POLYGON % (image_id, k))
                out.append((1, (x0, y0, x1, y1), polys))
            else:
                if list(seg["size"]) != [HH, WW]:
                    raise ValueError(_BAD_RLE_SIZE % (image_id, k, list(seg["size"]), [HH, WW]))
                counts = np.asarray(seg["counts"], np.int64) if isinstance(seg["counts"], list) else decode_counts(seg["counts"])
                out.append((2, (x0, y0, x1, y1), np.cumsum(counts)))
        return out

    def load(self, index):
        """One sample on the host: (pixels uint8 (h,w,3), objs (n,), boxes (n,4), image id)."""
        with self.open(index) as im:
            WW, HH = im.size
            pixels = np.asarray(im.convert("RGB"))
        objs, boxes = self.annotations(index, WW, HH)
        return pixels, torch.from_numpy(objs), torch.from_numpy(boxes), self.image_ids[index]


def pack_segmentations(segs, sizes, O):
    """The fields of ops.coco_masks for a batch, from the `segmentation_rows` of its samples, padded to O objects: kind,
    crop, sizes, (first, count) per object into the flat polygon offsets / vertices and the flat toggles."""
    B = len(segs)
    kind = np.zeros((B, O), np.uint8)
    crop = np.zeros((B, O, 4), np.int32)
    obj_poly, obj_runs = np.zeros((B, O, 2), np.int32), np.zeros((B, O, 2), np.int32)
    polys, runs, n_poly, n_tog = [], [], 0, 0
    for b, rows in enumerate(segs):
        for o, (what, c, payload) in enumerate(rows):
            kind[b, o], crop[b, o] = what, c
            if what == 1:
                obj_poly[b, o] = (n_poly, len(payload))
                polys += payload
                n_poly += len(payload)
            else:
                t = np.clip(payload, 0, 2 ** 31 - 1).astype(np.int32)      # toggles beyond the picture never matter
                obj_runs[b, o] = (n_tog, t.shape[0])
                runs.append(t)
                n_tog += t.shape[0]
    poly_off = np.zeros(n_poly + 1, np.int32)
    if polys:
        poly_off[1:] = np.cumsum([p.shape[0] for p in polys])
    return {"seg_kind": kind, "seg_crop": crop, "seg_sizes": np.ascontiguousarray(sizes, np.int64), "seg_obj_poly": obj_poly,
            "seg_poly_off": poly_off,
            "seg_poly_xy": np.concatenate(polys, 0) if polys else np.zeros((0, 2), np.float64),
            "seg_obj_runs": obj_runs, "seg_toggles": np.concatenate(runs) if runs else np.zeros(0, np.int32)}


def segmentation_fields(builder, indices, sizes, O):
    """`pack_segmentations` over the builder's samples; the per-sample rows (the strings' decode among them) are made in the
    builder's worker threads, which touch numpy only."""
    segs = list(builder.pool.map(lambda a: builder.ds.segmentation_rows(a[0], a[1][1], a[1][0]), zip(indices, sizes.tolist())))
    return pack_segmentations(segs, sizes, O)


def device_masks(ds, dev, p):
    """(masks, centres) of a batch whose second buffer carries `pack_segmentations`' fields: one launch of ops.coco_masks at
    the dataset's mask size, or at its working size for the centres alone when mask_size is 0 (masks None)."""
    from ... import ops
    return ops.coco_masks(dev["seg_kind"], dev["seg_crop"], dev["seg_sizes"], dev["boxes"], dev["seg_obj_poly"],
                          dev["seg_poly_off"], dev["seg_poly_xy"], dev["seg_obj_runs"], dev["seg_toggles"],
                          ds.mask_size or ds.default_mask_size, want_masks=bool(ds.mask_size), kind_host=p.seg_kind,
                          crop_host=p.seg_crop, sizes_host=p.seg_sizes, obj_poly_host=p.seg_obj_poly,
                          poly_off_host=p.seg_poly_off, poly_xy_host=p.seg_poly_xy, obj_runs_host=p.seg_obj_runs)


class CocoBatchBuilder(BatchBuilder):
    """Batches of a PackedCocoSceneGraphDataset (loader.BatchBuilder has the two halves of a batch): every picture goes up as
    RGB; the fields of its own are the category ids and the boxes over the decoded sizes, and no kernel of its own runs —
    unless the dataset reads segmentations: then their fields travel too and assemble launches ops.coco_masks."""

    def rows(self, indices, sizes, drawn):
        ann = [self.ds.annotations(i, w, h) for i, (h, w) in zip(indices, sizes.tolist())]
        O = max(a[0].shape[0] for a in ann)
        objs = np.zeros((len(ann), O, 1), np.int64)
        boxes = np.full((len(ann), O, 4), -1.0, np.float32)
        for b, (o, bx) in enumerate(ann):
            objs[b, :o.shape[0], 0] = o
            boxes[b, :bx.shape[0]] = bx
        seg = segmentation_fields(self, indices, sizes, O) if self.ds.segmentations else {}
        return {"objs": objs, "boxes": boxes, **seg}, {}

    def assemble(self, dev, p):
        if self.ds.segmentations:
            return dev["objs"], dev["boxes"], None, None, device_masks(self.ds, dev, p)
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
    segmentations = bool(getattr(args, "coco_segmentations", 0))
    if args.mask_size and not segmentations:
        raise NotImplementedError(_NO_MASKS % args.mask_size)
    inst = getattr(args, "coco_%s_instances_json" % split) or os.path.join(root, "annotations", "instances_%s2017.json" % split)
    stuff = getattr(args, "coco_%s_stuff_json" % split) or os.path.join(root, "annotations", "stuff_%s2017.json" % split)
    return PackedCocoSceneGraphDataset(
        image_dir, inst, stuff, image_size=args.image_size, mask_size=args.mask_size,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        min_object_size=args.min_object_size, min_objects=args.min_objects or 16, max_objects=args.max_objects or 1000,
        segmentations=segmentations)
