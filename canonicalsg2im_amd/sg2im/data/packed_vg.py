"""Visual Genome from a folder of pictures and a packed split file, with the input stage on the device (reference:
sg2im/data/packed_vg.py).

`PackedVGDataset` reads `vocab.json` and the split file and does what the reference's constructor does (:15-65): the
`min_objects` filter over every table (:52-58), `vocab["attributes"] = {"objects": object_name_to_idx}` with its reverse
(:60-64), the augmented relations (:65); `use_transitivity` / `use_converse` raise as there (:40-41).  `image_id` is the
integer stem of the picture's path (:78).  The tables stay numpy int32 on the host.

SPLIT FILE.  The arrays carry the names the reference's scripts/preprocess_packed_vg.py writes: object_names (N,MO),
object_boxes (N,MO,4) = x, y, w, h in pixels, objects_per_image (N,), relationship_subjects / _predicates / _objects (N,MR),
relationships_per_image (N,), image_paths (N,) str or bytes; other keys are ignored.  NAME.npz is read with numpy
(allow_pickle=False).  NAME.h5 is read through h5py, imported only then; where h5py is missing the error names the file and
tools/vg_h5_to_npz.py, which turns the one into the other on a machine that has h5py.  A path that does not exist is tried
with the other extension.  Only the .npz branch is tested: h5py is not installed where this package is built and tested.

`select(index, rng)` is the host half of __getitem__ (:86-137): which objects a sample keeps and its annotated rows.  The
reference decides with Python sets and `random.sample`; the same statements in the same order are made here, so the same
state of `rng` (anything with `.sample`, the `random` module included) gives the reference's own choice on one
interpreter version.  The reference's off-by-one is kept: a sample with more than max_objects - 1 related objects keeps
`max_objects` of them (:99-100), so it has max_objects + 1 rows with `__image__`.

Everything else of __getitem__ and vg_collate_fn runs on the device (`VGBatchBuilder`): the object ids, the boxes (pixel
boxes over the decoded picture's size, the reference's fp64 quotients bit for bit) and the padding in `ops.vg_rows`, Pillow's
resize, ToTensor and encode_image()'s Normalize(0.5, 0.5) in `ops.preprocess_images`, the `__image__` row and the canonical
graph over the annotated rows (csg_canon_general_*) in `collate.packed_batch`.

MASKS: the reference returns `masks = None` for this dataset (:143); `mask_size` must be 0."""
import json
import os
import random

import numpy as np
import torch

from . import register_augmented_relations
from .loader import BatchBuilder

VG_MEAN = VG_STD = 0.5                                     # encode_image(), sg2im/data/utils.py:13-14
VG_MAX_OBJECTS, VG_MIN_OBJECTS = 100, 16                   # sg2im/data/dataset_params.py:42-44
TABLES = ("object_names", "object_boxes", "objects_per_image", "relationship_subjects", "relationship_predicates",
          "relationship_objects", "relationships_per_image")

_NO_MASKS = ("PackedVGDataset: mask_size must be 0 (got %d): the reference returns masks = None for this dataset "
             "(sg2im/data/packed_vg.py:143)")
_NO_H5PY = ("%s is an HDF5 file and h5py cannot be imported here (%s).  Run `python tools/vg_h5_to_npz.py %s` on a machine "
            "that has h5py and pass the .npz it writes: that is read with numpy alone")


def split_file(path):
    """`path` when it exists, else the same path with the other of the two extensions (.npz / .h5) when that exists, else
    None."""
    if path and os.path.isfile(path):
        return path
    stem, ext = os.path.splitext(path or "")
    other = {".npz": ".h5", ".h5": ".npz"}.get(ext)
    if other and os.path.isfile(stem + other):
        return stem + other
    return None


def load_split(path):
    """The split file -> ({table name: int32 array}, [picture path str])."""
    found = split_file(path)
    if found is None:
        raise FileNotFoundError("no split file %s (nor with the other of .npz / .h5)" % path)
    if found.endswith(".npz"):
        with np.load(found, allow_pickle=False) as z:
            arrays = {k: z[k] for k in TABLES + ("image_paths",) if k in z.files}
    else:
        try:
            import h5py                        # only here: nothing else of the package needs it
        except ImportError as e:
            raise ImportError(_NO_H5PY % (found, e, found)) from e
        with h5py.File(found, "r") as f:
            arrays = {k: np.asarray(f[k]) for k in TABLES + ("image_paths",) if k in f}
    missing = [k for k in TABLES + ("image_paths",) if k not in arrays]
    if missing:
        raise KeyError("%s lacks %s" % (found, ", ".join(missing)))
    paths = [p.decode() if isinstance(p, (bytes, np.bytes_)) else str(p) for p in arrays.pop("image_paths").tolist()]
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in arrays.items()}, paths


class PackedVGDataset:
    def __init__(self, split_path, image_dir, vocab_json, image_size=(64, 64), mask_size=0, normalize_images=True,
                 min_objects=0, max_objects=1000, max_samples=None, include_relationships=True, use_orphaned_objects=True,
                 use_transitivity=False, use_converse=False):
        self.check_flags(use_transitivity, use_converse, mask_size, int(max_objects))
        self.image_dir = image_dir
        self.image_size = tuple(image_size)
        self.normalize_images = bool(normalize_images)
        self.min_objects, self.max_objects, self.max_samples = min_objects, int(max_objects), max_samples
        self.include_relationships = bool(include_relationships)
        self.use_orphaned_objects = bool(use_orphaned_objects)
        with open(vocab_json, "r") as f:
            self.vocab = json.load(f)
        self.num_objects = len(self.vocab["object_idx_to_name"])
        if self.vocab["object_name_to_idx"].get("__image__") != 0:
            raise ValueError("%s: __image__ must be object 0 (the collate pads objects with 0); it is %r" % (
                vocab_json, self.vocab["object_name_to_idx"].get("__image__")))
        self.data, self.image_paths = load_split(split_path)
        n = len(self.data["objects_per_image"])
        if len(self.image_paths) != n or any(len(v) != n for v in self.data.values()):
            raise ValueError("%s: the tables and image_paths differ in their first dimension" % split_path)
        if min_objects and min_objects > 0:                                             # :52-58
            keep = np.nonzero(self.data["objects_per_image"] >= min_objects)[0]
            self.data = {k: np.ascontiguousarray(v[keep]) for k, v in self.data.items()}
            self.image_paths = [self.image_paths[i] for i in keep]
        self.image_ids = [int(p.split("/")[-1].split(".")[0]) for p in self.image_paths]  # :78
        self.vocab["attributes"] = {"objects": self.vocab["object_name_to_idx"]}        # :60-64
        self.vocab["reverse_attributes"] = {a: {v: k for k, v in t.items()} for a, t in self.vocab["attributes"].items()}
        self.add_predicates()

    def check_flags(self, use_transitivity, use_converse, mask_size, max_objects):
        """What the constructor refuses before it reads a file."""
        if use_transitivity or use_converse:
            raise NotImplementedError("PackedVGDataset: use_transitivity / use_converse are not implemented, as in the "
                                      "reference (sg2im/data/packed_vg.py:40-41)")
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)

    def add_predicates(self):
        """The predicates the constructor adds to vocab.json's."""
        register_augmented_relations(self.vocab)                                        # :65

    def __len__(self):
        n = len(self.image_paths)
        return n if self.max_samples is None else min(n, self.max_samples)

    def open(self, index):
        """The opened picture (header read, pixels not yet decoded) of sample `index`."""
        from PIL import Image                  # only here: importing the package never needs PIL
        return Image.open(os.path.join(self.image_dir, self.image_paths[index]))

    def select(self, index, rng=random):
        """-> (the chosen objects' indices into the sample's table rows, in the reference's order; the annotated rows
        [[s', p, o']] both of whose ends were chosen, in file order, as positions in that list).  :86-104, :127-137."""
        d = self.data
        n_rel = int(d["relationships_per_image"][index])
        subjects = d["relationship_subjects"][index, :n_rel].tolist()
        predicates = d["relationship_predicates"][index, :n_rel].tolist()
        objects = d["relationship_objects"][index, :n_rel].tolist()
        with_rels = set()                       # the reference's statements in its order: a set's iteration order depends on
        without_rels = set(range(int(d["objects_per_image"][index])))       # how it was filled
        for s, o in zip(subjects, objects):
            with_rels.add(s)
            with_rels.add(o)
            without_rels.discard(s)
            without_rels.discard(o)
        chosen = list(with_rels)
        without_rels = list(without_rels)
        if len(chosen) > self.max_objects - 1:
            chosen = rng.sample(chosen, self.max_objects)                   # max_objects, not minus one: the reference's
        if len(chosen) < self.max_objects - 1 and self.use_orphaned_objects:
            missing = min(self.max_objects - 1 - len(chosen), len(without_rels))
            chosen += rng.sample(without_rels, missing)
        rows = []
        if self.include_relationships:
            position = {obj: i for i, obj in enumerate(chosen)}
            for s, p, o in zip(subjects, predicates, objects):
                s, o = position.get(s), position.get(o)
                if s is not None and o is not None:
                    rows.append([s, p, o])
        return chosen, rows

    def load(self, index, rng=random):
        """One sample on the host: (pixels uint8 (h,w,3), rows int32 (n,5) = name, x, y, w, h, annotated rows int64 (r,3),
        image id)."""
        with self.open(index) as im:
            pixels = np.asarray(im.convert("RGB"))
        chosen, rel = self.select(index, rng)
        rows = np.concatenate([self.data["object_names"][index, chosen, None], self.data["object_boxes"][index, chosen]], 1)
        return pixels, rows.astype(np.int32), np.asarray(rel, np.int64).reshape(-1, 3), self.image_ids[index]


class VGBatchBuilder(BatchBuilder):
    """Batches of a PackedVGDataset (loader.BatchBuilder has the two halves of a batch): RGBA pictures go up as 4-byte pixels,
    any mode but RGB and RGBA (L, CMYK, P: Visual Genome has some of each) is converted to RGB on the host first.  Before
    anything else start() calls `select` for every sample in batch order on the consumer's thread (the order decides what
    the random stream gives whom, so the workers do not do it).  The fields of its own are the counts, the decoded sizes
    (HH, WW) (int64) and the gathered rows (B,O,5) int32 = name, x, y, w, h (-1 in padding rows), from which ops.vg_rows
    makes objects and boxes; the annotated rows and the counts reach collate.packed_batch as host tensors;
    Normalize(0.5, 0.5).

    `rng`: where `select` draws; by default a random.Random of the builder's own, seeded from (0, rank).  A resumed run
    starts it afresh: its epoch order is the interrupted run's, its object sampling is not."""

    keep_rgba = takes_rng = True
    mean, std = VG_MEAN, VG_STD

    def __init__(self, dataset, args, trainer, device, num_workers=1, rng=None):
        super().__init__(dataset, args, trainer, device, num_workers=num_workers)
        if rng is None:
            from ... import dist
            rng = random.Random((0 << 32) | dist.rank())
        self.rng = rng

    def draw(self, indices):
        picked = [self.ds.select(i, self.rng) for i in indices]            # in batch order: the stream's order
        if max(len(chosen) for chosen, _ in picked) < 1:
            raise ValueError("a batch of samples without objects")
        return picked

    def rows(self, indices, sizes, picked):
        ds = self.ds
        B, O, R = len(picked), max(len(chosen) for chosen, _ in picked), max(len(rel) for _, rel in picked)
        rows = np.full((B, O, 5), -1, np.int32)
        rel = torch.zeros((B, R, 3), dtype=torch.int64)
        rel[:, :, 1] = ds.vocab["pred_name_to_idx"]["__padding__"]
        for b, (i, (chosen, annotated)) in enumerate(zip(indices, picked)):
            rows[b, :len(chosen), 0] = ds.data["object_names"][i, chosen]
            rows[b, :len(chosen), 1:] = ds.data["object_boxes"][i, chosen]
            if annotated:
                rel[b, :len(annotated)] = torch.as_tensor(annotated, dtype=torch.int64)
        return {"counts": np.asarray([len(chosen) for chosen, _ in picked], np.int64), "sizes": sizes, "rows": rows}, \
            {"rel": rel}

    def assemble(self, dev, p):
        from ... import ops
        objs, boxes = ops.vg_rows(dev["rows"], dev["sizes"], dev["counts"], self.ds.num_objects, rows_host=p.rows,
                                  sizes_host=p.sizes, counts_host=p.counts)
        return objs, boxes, p.rel, p.counts

    def host_objs(self, p):
        names = p.rows[..., :1].to(torch.int64)                            # -1 at and beyond a sample's count: 0, as vg_rows
        return names.clamp_(min=0)


PackedVGDataset.builder_class = VGBatchBuilder


def split_image_dir(args, split):
    """Where the pictures are looked for: --vg_image_dir when it exists, else <dataroot>/vg/images (every split's)."""
    return args.vg_image_dir if args.vg_image_dir and os.path.isdir(args.vg_image_dir) else os.path.join(args.dataroot, "vg", "images")


def build_vg_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory or its
    split file is not found.  Each path is the flag's value when that exists (--vg_image_dir, --train_h5 / --val_h5,
    --vocab_json), else the reference's layout under --dataroot (sg2im/data/dataset_params.py:40-60): <dataroot>/vg/images,
    /train.h5 or /val.h5, /vocab.json; the split file is taken with either extension, .npz or .h5.  max_objects = 100 and
    min_objects = 16 as there, unless --max_objects / --min_objects say otherwise."""
    base = os.path.join(args.dataroot, "vg")
    image_dir = split_image_dir(args, split)
    given = getattr(args, "%s_h5" % split)
    found = split_file(given) or split_file(os.path.join(base, "%s.h5" % split))
    if not os.path.isdir(image_dir) or found is None:
        return None
    if args.mask_size:
        raise NotImplementedError(_NO_MASKS % args.mask_size)
    vocab_json = args.vocab_json if args.vocab_json and os.path.isfile(args.vocab_json) else os.path.join(base, "vocab.json")
    return PackedVGDataset(
        found, image_dir, vocab_json, image_size=args.image_size, mask_size=args.mask_size,
        min_objects=VG_MIN_OBJECTS if args.min_objects is None else args.min_objects,
        max_objects=args.max_objects or VG_MAX_OBJECTS,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        include_relationships=bool(args.include_relationships), use_orphaned_objects=bool(args.vg_use_orphaned_objects),
        use_transitivity=bool(args.use_transitivity), use_converse=bool(args.use_converse))
