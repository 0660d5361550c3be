"""CLEVR from a folder of renders, with the input stage on the device (reference: sg2im/data/packed_clevr_dialog.py).

`PackedClevrDataset` reads the scenes file (`scenes/CLEVR_{mode}_scenes.json`) and keeps the reference's vocabulary
(:113-143): the four attribute tables shape / color / material / size of 4 / 9 / 3 / 3 rows, `use_object_embedding = False`,
the `object_name_to_idx` keys its loop builds ("<label>_<running index>", "__image__" at 0) and the eight packed predicates.
An object is a row of four attribute ids in the reference's column order — shape, color, material, size: the order of the
attribute dict (the collate's `sorted(attributes)` discards its result, :292).  `image_id` is the scene's `image_index`.
The only filters are `dense_scenes` (min_objects < n < max_objects, both strict, :226-240) and `max_samples`.  Where the
reference's dialog file exists, the picture of sample i is `split` / `image_filename` of ITS entry i, as in the reference
(:177-178); otherwise of the scene record itself.

What the host does per image is: open the file, copy the decoded bytes into a pinned staging buffer (RGBA renders as they
are, 4 bytes per pixel: no convert('RGB') pass), copy the scene's raw numbers.  Everything else of the reference's
`__getitem__` and collate runs on the device (`ClevrBatchBuilder`): the boxes from the scene geometry in `ops.clevr_boxes`
(the reference's fp64 formula, bit for bit), Pillow's resize, ToTensor and encode_image()'s Normalize(0.5, 0.5) in
`ops.preprocess_images`, the `__image__` row, the canonical graph and the padding in `collate.packed_batch`.  Object centres
are box centres, as in the reference (:191-198): the graphs are the reference's graphs.

MASKS: the reference returns `masks = None` for this dataset (:212); `mask_size` must be 0."""
import json
import os

import numpy as np
import torch

from . import register_augmented_relations
from .loader import BatchBuilder

CLEVR_MEAN = CLEVR_STD = 0.5                               # encode_image(), sg2im/data/utils.py:13-14
ATTRIBUTES = {                                             # packed_clevr_dialog.py:121-125, in this order
    "shape": {"__image__": 0, "cube": 1, "sphere": 2, "cylinder": 3},
    "color": {"__image__": 0, "gray": 1, "red": 2, "blue": 3, "green": 4, "brown": 5, "purple": 6, "cyan": 7, "yellow": 8},
    "material": {"__image__": 0, "rubber": 1, "metal": 2},
    "size": {"__image__": 0, "small": 1, "large": 2},
}

_NO_MASKS = ("PackedClevrDataset: mask_size must be 0 (got %d): the reference returns masks = None for this dataset "
             "(sg2im/data/packed_clevr_dialog.py:212)")


def clevr_vocab(predicates=None):
    """The vocabulary of packed_clevr_dialog.py:113-143; with `predicates` (names by id) those are its predicate table, in
    place of the eight packed ones."""
    vocab = {"use_object_embedding": False}
    if predicates is None:
        register_augmented_relations(vocab)
    else:
        vocab["pred_name_to_idx"] = {name: i for i, name in enumerate(predicates)}
        vocab["pred_idx_to_name"] = list(predicates)
    vocab["attributes"] = {attr: dict(table) for attr, table in ATTRIBUTES.items()}
    vocab["reverse_attributes"] = {attr: {v: k for k, v in table.items()} for attr, table in ATTRIBUTES.items()}
    vocab["object_name_to_idx"] = {}
    ind = 0
    for attr in vocab["attributes"]:
        for label in vocab["attributes"][attr]:
            vocab["object_name_to_idx"][label if ind == 0 else "{}_{}".format(label, ind)] = ind
            ind += 1
    vocab["object_idx_to_name"] = {v: k for k, v in vocab["object_name_to_idx"].items()}
    return vocab


class PackedClevrDataset:
    def __init__(self, scenes_json, image_dir, dialog_json=None, split_dirs=True, image_size=(64, 64), mask_size=0,
                 normalize_images=True, max_samples=None, dense_scenes=False, min_objects=10, max_objects=10):
        """`image_dir`: with split_dirs the reference's <base>/images, under which a picture is <split>/<image_filename>;
        without, the directory of the pictures themselves.  `dialog_json`: the reference's clevr_dialog_{mode}_raw.json,
        read when the file exists."""
        self.check_flags(mask_size)
        self.image_dir = image_dir
        self.split_dirs = bool(split_dirs)
        self.image_size = tuple(image_size)
        self.normalize_images = bool(normalize_images)
        self.max_samples = max_samples
        self.vocab = self.make_vocab()
        with open(scenes_json, "r") as f:
            self.scenes = json.load(f)["scenes"]
        entries = self.scenes
        if dialog_json is not None and os.path.isfile(dialog_json):
            with open(dialog_json, "r") as f:
                entries = json.load(f)
        if dense_scenes:                                   # keep_dense_scenes: scene and dialog entry by the same index
            keep = [i for i, s in enumerate(self.scenes) if self.is_dense(len(s["objects"]), min_objects, max_objects)]
            entries = [entries[i] for i in keep]
            self.scenes = [self.scenes[i] for i in keep]
        self.image_paths = [os.path.join(e["split"], e["image_filename"]) if self.split_dirs else e["image_filename"]
                            for e in entries[:len(self.scenes)]]
        if len(self.image_paths) != len(self.scenes):
            raise ValueError("the dialog file has %d entries for %d scenes" % (len(self.image_paths), len(self.scenes)))
        self.image_ids = [int(s["image_index"]) for s in self.scenes]

    def check_flags(self, mask_size):
        """What the constructor refuses before it reads a file."""
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)

    def make_vocab(self):
        return clevr_vocab()

    def is_dense(self, n, min_objects, max_objects):
        """Whether `dense_scenes` keeps a scene of n objects (:226-240)."""
        return min_objects < n < max_objects

    def __len__(self):
        return len(self.scenes) if self.max_samples is None else min(len(self.scenes), self.max_samples)

    def open(self, index):
        """The opened picture (header read, pixels not yet decoded) of sample `index`."""
        from PIL import Image                  # only here: importing the package never needs PIL
        return Image.open(os.path.join(self.image_dir, self.image_paths[index]))

    def annotations(self, index):
        """The raw numbers of scene `index`: objs int64 (n,4) = shape, color, material, size ids; geom fp64 (n,5) = pixel x,
        pixel y, 3d x, y, z; rot fp64 (2,) = directions['right'][:2].  The boxes follow from geom and rot on the device."""
        scene = self.scenes[index]
        rows = scene["objects"]
        objs = np.asarray([[table[o[attr]] for attr, table in ATTRIBUTES.items()] for o in rows], np.int64).reshape(-1, 4)
        geom = np.asarray([[o["pixel_coords"][0], o["pixel_coords"][1]] + list(o["3d_coords"]) for o in rows],
                          np.float64).reshape(-1, 5)
        rot = np.asarray(scene["directions"]["right"][:2], np.float64)
        return objs, geom, rot

    def load(self, index):
        """One sample on the host: (pixels uint8 (h,w,3), objs (n,4), geom (n,5), rot (2,), image id)."""
        with self.open(index) as im:
            pixels = np.asarray(im.convert("RGB"))
        objs, geom, rot = self.annotations(index)[:3]
        return pixels, torch.from_numpy(objs), torch.from_numpy(geom), torch.from_numpy(rot), self.image_ids[index]


class ClevrBatchBuilder(BatchBuilder):
    """Batches of a PackedClevrDataset (loader.BatchBuilder has the two halves of a batch): RGBA renders go up as 4-byte
    pixels; the fields of its own are the object counts, the attribute rows (int64) and the scene numbers (fp64: geometry,
    rotation), from which ops.clevr_boxes makes the boxes; Normalize(0.5, 0.5)."""

    keep_rgba = True
    mean, std = CLEVR_MEAN, CLEVR_STD

    def rows(self, indices, sizes, drawn):
        return self.fields_of([self.ds.annotations(i) for i in indices]), {}

    def fields_of(self, ann):
        """The second buffer's fields from the samples' annotations (objs, geom, rot, ...), padded to the batch's O."""
        O = max(a[0].shape[0] for a in ann)
        if O < 1:
            raise ValueError("a batch of scenes without objects")
        objs = np.zeros((len(ann), O, 4), np.int64)
        geom = np.zeros((len(ann), O, 5), np.float64)
        for b, a in enumerate(ann):
            objs[b, :a[0].shape[0]] = a[0]
            geom[b, :a[1].shape[0]] = a[1]
        return {"counts": np.asarray([a[0].shape[0] for a in ann], np.int64), "objs": objs, "geom": geom,
                "rot": np.stack([a[2] for a in ann])}

    def assemble(self, dev, p):
        from ... import ops
        boxes = ops.clevr_boxes(dev["geom"], dev["objs"], dev["rot"], dev["counts"], objs_host=p.objs, counts_host=p.counts)
        return dev["objs"], boxes, None, None


PackedClevrDataset.builder_class = ClevrBatchBuilder


def split_image_dir(args, split):
    """Where the split's pictures are looked for: --clevr_<split>_image_dir, else the reference's layout under --dataroot."""
    return getattr(args, "clevr_%s_image_dir" % split) or os.path.join(args.dataroot, "CLEVR", "CLEVR_Dialog", "images", split)


def build_clevr_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory does not
    exist.  Paths: by default the reference's layout under --dataroot (sg2im/data/dataset_params.py:92-109): base =
    <dataroot>/CLEVR/CLEVR_Dialog, scenes base/scenes/CLEVR_<split>_scenes.json, pictures base/images/<entry's split>/<file
    name>, dialog file base/clevr_dialog_<split>_raw.json when present.  --clevr_<split>_scenes_json names another scenes
    file; --clevr_<split>_image_dir names the directory that holds the split's pictures themselves."""
    base = os.path.join(args.dataroot, "CLEVR", "CLEVR_Dialog")
    given = getattr(args, "clevr_%s_image_dir" % split)
    image_dir = split_image_dir(args, split)
    if not os.path.isdir(image_dir):
        return None
    if args.mask_size:
        raise NotImplementedError(_NO_MASKS % args.mask_size)
    scenes = getattr(args, "clevr_%s_scenes_json" % split) or os.path.join(base, "scenes", "CLEVR_%s_scenes.json" % split)
    return PackedClevrDataset(
        scenes, given or os.path.join(base, "images"), dialog_json=os.path.join(base, "clevr_dialog_%s_raw.json" % split),
        split_dirs=not given, image_size=args.image_size, mask_size=args.mask_size,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        dense_scenes=bool(args.dense_scenes), min_objects=args.min_objects or 0, max_objects=args.max_objects or 1000)
