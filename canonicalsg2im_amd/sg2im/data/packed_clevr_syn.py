"""Synthetic CLEVR scenes with more objects than any training picture has: the dataset of the reference's large-graph
generalisation run (`packed_clevr_syn`: sg2im/data/packed_clevr_dialog.py:337-515, the scenes of `create_packed_sgs`, read by
scripts/generate_clevr.py).  There is no folder and no picture: a scene is a list of objects — color, size, shape, material
drawn uniformly — and their boxes, squares of side 0.1 (small) or 0.2 (large) placed uniformly inside the picture.

`SynClevrScenes(min_objects, max_objects, max_samples, seed)` draws the scenes in the reference's order: per scene one
`randint(min, max)`, then per object four `randint` draws (color, size, shape, material) from a `random.Random(seed)`, then
per object one `uniform(0, 1 - size, size=2)` from a `np.random.RandomState(seed)` — the streams of the reference's global
`random.seed(seed)` and `np.random.seed(seed)`, so with equal seeds the scenes are the reference's, fp64 value for value.
`scenes_json` names a plain JSON file of scenes: it is read in place of drawing when it exists, written otherwise, which is
how two checkpoints see identical scenes (the reference keeps a pickle).

Batches (`SynClevrBatches`) carry no picture: imgs = None, masks = None, image ids int64 (`image_index` is str(j)).  The
object rows (shape, color, material, size ids, the vocabulary's column order) and the fp32 boxes are padded on the host —
rows of 0 and boxes of -1 — uploaded once, and go through `collate.packed_batch`, which appends the `__image__` row and
builds the canonical graph on the device.  The object centres are the reference's: `x0 + 0.5 * w` in Python fp64, THEN
rounded to fp32 (packed_clevr_dialog.py:427-434) — not the centres of the fp32 boxes, which differ in the last bit for
some objects — and are handed to `packed_batch(..., centers=...)`."""
import json
import os
import random

import numpy as np
import torch

from .loader import HostBatch
from .packed_clevr import ATTRIBUTES, clevr_vocab

MAX_OBJECTS = 255                                          # 256 graph rows with `__image__` (canonical_triplets' limit)
SIZES = {"small": 0.1, "large": 0.2}                       # packed_clevr_dialog.py:490-494
_DRAW_ORDER = ("color", "size", "shape", "material")       # :476-483

_NO_MASKS = ("SynClevrScenes: mask_size must be 0 (got %d): the reference returns masks = None for this dataset "
             "(sg2im/data/packed_clevr_dialog.py:448)")
NO_VALIDATION = ("--dataset packed_clevr_syn cannot be validated on: its samples carry no picture, and the validation "
                 "passes compare pictures; its run is python -m canonicalsg2im_amd.scripts.sample --dataset packed_clevr_syn")
NO_TRAINING = ("--dataset packed_clevr_syn cannot be trained on: its samples carry no picture (the reference's return "
                "image = None, sg2im/data/packed_clevr_dialog.py:449); it is the dataset of the large-graph run, "
                "python -m canonicalsg2im_amd.scripts.sample --dataset packed_clevr_syn")


def draw_scenes(min_objects, max_objects, max_samples, seed):
    """`create_packed_sgs` (:464-515) without its relations: [{"image_index", "objects", "boxes"}]."""
    rnd, nrs = random.Random(seed), np.random.RandomState(seed)
    reverse = {attr: {v: k for k, v in table.items()} for attr, table in ATTRIBUTES.items()}
    scenes = []
    for j in range(max_samples):
        n = rnd.randint(min_objects, max_objects)
        objects = []
        for _ in range(n):
            drawn = {attr: reverse[attr][rnd.randint(1, len(ATTRIBUTES[attr]) - 1)] for attr in _DRAW_ORDER}
            objects.append(drawn)
        boxes = []
        for obj in objects:
            side = SIZES[obj["size"]]
            x0, y0 = nrs.uniform(0, 1 - side, size=2)
            boxes.append([float(x0), float(y0), side, side])
        scenes.append({"image_index": str(j), "objects": objects, "boxes": boxes})
    return scenes


def check_scenes(scenes, where):
    """What a scenes file must hold, before anything is made of it: ValueError("<where>: scene <j>: ...")."""
    if not isinstance(scenes, list) or not scenes:
        raise ValueError("%s: a non-empty list of scenes is needed" % where)
    for j, s in enumerate(scenes):
        bad = lambda what, j=j: ValueError("%s: scene %d: %s" % (where, j, what))
        if not isinstance(s, dict) or not isinstance(s.get("objects"), list) or not isinstance(s.get("boxes"), list):
            raise bad("a scene is {\"image_index\": ..., \"objects\": [...], \"boxes\": [...]}")
        if not 1 <= len(s["objects"]) <= MAX_OBJECTS or len(s["boxes"]) != len(s["objects"]):
            raise bad("%d objects and %d boxes: 1 .. %d objects, a box each" % (len(s["objects"]), len(s["boxes"]), MAX_OBJECTS))
        try:
            int(s["image_index"])
        except (KeyError, TypeError, ValueError):
            raise bad("image_index %r is not a number" % (s.get("image_index"),))
        for obj in s["objects"]:
            for attr, table in ATTRIBUTES.items():
                if not isinstance(obj, dict) or obj.get(attr) not in table or obj.get(attr) == "__image__":
                    raise bad("object %r has no %s among %s" % (obj, attr, [k for k in table if k != "__image__"]))
        for box in s["boxes"]:
            if not isinstance(box, list) or len(box) != 4 or not all(isinstance(v, (int, float)) and not isinstance(v, bool)
                                                                     and v == v and abs(v) != float("inf") for v in box):
                raise bad("box %r is not four finite numbers" % (box,))
    if len({int(s["image_index"]) for s in scenes}) != len(scenes):
        raise ValueError("%s: an image_index a second time: it would overwrite a file" % where)


class SynClevrScenes:
    def __init__(self, min_objects=15, max_objects=30, max_samples=1000, seed=0, scenes_json=None, mask_size=0):
        """The defaults are scripts/generate_clevr.py's.  `scenes_json`: read when the file exists (the four numbers
        before it then say nothing), else written with the scenes drawn."""
        self.check_flags(min_objects, max_objects, max_samples, mask_size)
        self.min_objects, self.max_objects, self.seed = int(min_objects), int(max_objects), int(seed)
        self.vocab = clevr_vocab()
        self.scenes_json = scenes_json
        self.loaded = bool(scenes_json) and os.path.isfile(scenes_json)
        if self.loaded:
            with open(scenes_json, "r") as f:
                held = json.load(f)
            self.scenes = held.get("scenes") if isinstance(held, dict) else held
            check_scenes(self.scenes, scenes_json)
            if isinstance(held, dict) and isinstance(held.get("seed"), int):
                self.seed = held["seed"]
        else:
            self.scenes = draw_scenes(self.min_objects, self.max_objects, int(max_samples), self.seed)
            if scenes_json:
                self.save(scenes_json)
        self.image_ids = [int(s["image_index"]) for s in self.scenes]
        self.image_dir = "no folder (scenes %s)" % ("of %s" % scenes_json if self.loaded else "drawn from seed %d" % self.seed)

    @staticmethod
    def check_flags(min_objects, max_objects, max_samples, mask_size):
        """What the constructor refuses before it draws or reads anything."""
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)
        if min_objects < 1:
            raise ValueError("SynClevrScenes: min_objects must be at least 1 (got %d): a scene without objects has no graph"
                             % min_objects)
        if max_objects > MAX_OBJECTS:
            raise ValueError("SynClevrScenes: max_objects must be at most %d (got %d): the canonical graph takes 256 rows with "
                             "`__image__`" % (MAX_OBJECTS, max_objects))
        if max_objects < min_objects:
            raise ValueError("SynClevrScenes: max_objects %d is below min_objects %d" % (max_objects, min_objects))
        if max_samples < 1:
            raise ValueError("SynClevrScenes: max_samples must be at least 1 (got %d)" % max_samples)

    def save(self, path):
        """Plain JSON; Python writes a float's shortest repr, which reads back as the same fp64."""
        with open(path, "w") as f:
            json.dump({"seed": self.seed, "min_objects": self.min_objects, "max_objects": self.max_objects,
                       "scenes": self.scenes}, f)

    def __len__(self):
        return len(self.scenes)

    def annotations(self, index):
        """Scene `index` on the host: objs int64 (n,4) = shape, color, material, size ids; boxes fp64 (n,4) xywh; centres
        fp32 (n,2), each `x0 + 0.5 * w` in fp64 and then rounded, as the reference forms them."""
        scene = self.scenes[index]
        objs = np.asarray([[table[o[attr]] for attr, table in ATTRIBUTES.items()] for o in scene["objects"]], np.int64)
        boxes = np.asarray(scene["boxes"], np.float64).reshape(-1, 4)
        centres = np.asarray([[x0 + 0.5 * w, y0 + 0.5 * h] for x0, y0, w, h in scene["boxes"]], np.float64).astype(np.float32)
        return objs.reshape(-1, 4), boxes, centres.reshape(-1, 2)


class SynClevrBatches:
    """Batches of a SynClevrScenes: `batches(index_lists)` yields the trainer's 8-tuple on the device as a
    loader.HostBatch (its object ids on the host too), imgs and masks None.  No threads and no files: `close()` is there
    for the callers that close a builder."""

    takes_rng = False

    def __init__(self, ds, args, trainer, dev, num_workers=0):
        self.ds, self.args, self.trainer, self.dev = ds, args, trainer, dev
        self.num_workers = 0

    def host_batch(self, indices):
        """The padded host tensors of the scenes `indices`: (objs (B,O,4) int64, boxes (B,O,4) fp32, centres (B,O,2) fp32,
        counts (B,) int64, image ids (B,) int64)."""
        ann = [self.ds.annotations(i) for i in indices]
        B, O = len(ann), max(a[0].shape[0] for a in ann)
        objs = np.zeros((B, O, 4), np.int64)
        boxes = np.full((B, O, 4), -1.0, np.float32)
        centres = np.full((B, O, 2), -1.5, np.float32)     # a padding row's box centre; never a real object's
        for b, (o, bx, ce) in enumerate(ann):
            n = o.shape[0]
            objs[b, :n], boxes[b, :n], centres[b, :n] = o, bx.astype(np.float32), ce
        counts = np.asarray([a[0].shape[0] for a in ann], np.int64)
        ids = np.asarray([self.ds.image_ids[i] for i in indices], np.int64)
        return tuple(torch.from_numpy(x) for x in (objs, boxes, centres, counts, ids))

    def batches(self, index_lists):
        from .collate import packed_batch
        for indices in index_lists:
            objs, boxes, centres, counts, ids = self.host_batch(indices)
            batch = packed_batch(self.args, self.trainer, [None, objs, boxes, None, None, None, None, ids], self.dev,
                                 counts=counts, centers=centres)
            image_row = torch.zeros((objs.shape[0], 1, objs.shape[2]), dtype=torch.int64)
            yield HostBatch(batch, torch.cat([objs, image_row], 1))

    def close(self):
        pass


SynClevrScenes.builder_class = SynClevrBatches


def split_image_dir(args, split):
    """For `looked_for`: there is no folder to look for."""
    return "no folder: --dataset packed_clevr_syn draws its scenes from --seed, or reads them from --scenes"


def build_clevr_syn_dataset(args, split):
    """The scenes named by the command line: --min_objects (15), --max_objects (30), --max_samples (1000), --seed (0),
    --scenes FILE — scripts/generate_clevr.py's defaults.  The same scenes for every split: they are not data to fit."""
    given = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)
    return SynClevrScenes(given("min_objects", 15), given("max_objects", 30), given("max_samples", 1000), given("seed", 0),
                          scenes_json=getattr(args, "scenes", None), mask_size=args.mask_size)
