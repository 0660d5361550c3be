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
from .collate import packed_batch
from .loader import BatchBuilder, _Pending

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
        if use_transitivity or use_converse:
            raise NotImplementedError("PackedVGDataset: use_transitivity / use_converse are not implemented, as in the "
                                      "reference (sg2im/data/packed_vg.py:40-41)")
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)
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
    """Batches of a PackedVGDataset as the 8-tuple Trainer.step takes (loader.BatchBuilder has the staging, the look-ahead
    and the rule that the workers make no HIP call).

    start(indices), on the consumer's thread: `select` for every sample in batch order (the order decides what the random
    stream gives whom, so the workers do not do it); the pictures are opened for sizes and modes and decoded by the worker
    threads into a pinned buffer — RGB as 3-byte pixels, RGBA as 4-byte pixels, any other mode (L, CMYK, P: Visual Genome
    has some of each) converted to RGB on the host first; every picture starts on a 4-byte boundary.  The descriptor, the
    image ids, the counts, the decoded sizes (HH, WW) (int64) and the gathered rows (B,O,5) int32 = name, x, y, w, h (-1 in
    padding rows) are laid out in a second one.  finish(pending): ONE copy of each, ops.vg_rows, ops.preprocess_images with
    Normalize(0.5, 0.5), collate.packed_batch with the annotated rows and the counts as host tensors.

    `rng`: where `select` draws; by default a random.Random of the builder's own, seeded from (0, rank).  A resumed run
    starts it afresh: its epoch order is the interrupted run's, its object sampling is not."""

    def __init__(self, dataset, args, trainer, device, num_workers=1, rng=None):
        super().__init__(dataset, args, trainer, device, num_workers=num_workers)
        if rng is None:
            from ... import dist
            rng = random.Random((0 << 32) | dist.rank())
        self.rng = rng

    @staticmethod
    def _decode(im, dst, mode):
        try:
            dst[:] = np.asarray(im if im.mode == mode else im.convert(mode)).reshape(-1)
        finally:
            im.close()

    def start(self, indices):
        """The host half.  Called by the consumer's thread between two steps: the one HIP call it can make, the pinned
        allocation when a staging buffer has to grow, is made here and not by a worker."""
        B = len(indices)
        ds = self.ds
        picked = [ds.select(i, self.rng) for i in indices]                 # in batch order: the stream's order
        O = max(len(chosen) for chosen, _ in picked)
        if O < 1:
            raise ValueError("a batch of samples without objects")
        R = max(len(rel) for _, rel in picked)
        slot = self._take_slot()
        opened = list(self.pool.map(ds.open, indices))                     # headers: sizes and modes
        modes = ["RGBA" if im.mode == "RGBA" else "RGB" for im in opened]
        desc = np.zeros((B, 4), np.int64)
        end = 0
        for b, (im, mode) in enumerate(zip(opened, modes)):
            desc[b] = (-(-end // 4) * 4, im.size[1], im.size[0], len(mode))
            end = int(desc[b, 0] + desc[b, 1] * desc[b, 2] * desc[b, 3])
        stage = self.pixels[slot].take(end)[:end]
        host = stage.numpy()                                               # the workers write through numpy: no torch call
        futures = [self.pool.submit(self._decode, im, host[desc[b, 0]:desc[b, 0] + desc[b, 1] * desc[b, 2] * desc[b, 3]], mode)
                   for b, (im, mode) in enumerate(zip(opened, modes))]
        # descriptor | image ids | counts | sizes (int64), then the rows (int32): one buffer, one copy
        n64 = 4 * B + B + B + 2 * B
        nbytes = 8 * n64 + 4 * 5 * B * O
        meta = self.meta[slot].take(nbytes)[:nbytes]
        i64 = meta[:8 * n64].view(torch.int64)
        rows_host = meta[8 * n64:].view(torch.int32).view(B, O, 5)
        i64[:4 * B] = torch.from_numpy(desc.reshape(-1))
        i64[4 * B:5 * B] = torch.as_tensor([ds.image_ids[i] for i in indices], dtype=torch.int64)
        counts_host = i64[5 * B:6 * B]
        sizes_host = i64[6 * B:8 * B].view(B, 2)
        sizes_host.copy_(torch.from_numpy(desc[:, 1:3]))                   # (HH, WW) of the decoded pictures
        rows_np = np.full((B, O, 5), -1, np.int32)
        rel = torch.zeros((B, R, 3), dtype=torch.int64)
        rel[:, :, 1] = ds.vocab["pred_name_to_idx"]["__padding__"]
        for b, (i, (chosen, rows)) in enumerate(zip(indices, picked)):
            n = len(chosen)
            counts_host[b] = n
            rows_np[b, :n, 0] = ds.data["object_names"][i, chosen]
            rows_np[b, :n, 1:] = ds.data["object_boxes"][i, chosen]
            if rows:
                rel[b, :len(rows)] = torch.as_tensor(rows, dtype=torch.int64)
        rows_host.copy_(torch.from_numpy(rows_np))
        return _Pending(futures=futures, slot=slot, stage=stage, meta=meta, desc=torch.from_numpy(desc), rows=rows_host.clone(),
                        sizes=sizes_host.clone(), counts=counts_host.clone(), rel=rel, B=B, O=O, n64=n64)

    def finish(self, p):
        """The device half, enqueued on the current stream."""
        from ... import ops
        B, O, n64 = p.B, p.O, p.n64
        src, meta_dev = self._upload(p)
        i64_dev = meta_dev[:8 * n64].view(torch.int64)
        rows_dev = meta_dev[8 * n64:].view(torch.int32).view(B, O, 5)
        objs, boxes = ops.vg_rows(rows_dev, i64_dev[6 * B:8 * B].view(B, 2), i64_dev[5 * B:6 * B], self.ds.num_objects,
                                  rows_host=p.rows, sizes_host=p.sizes, counts_host=p.counts)
        H, W = self.ds.image_size
        imgs = ops.preprocess_images(src, i64_dev[:4 * B].view(B, 4), H, W, normalize=self.ds.normalize_images,
                                     desc_host=p.desc, mean=VG_MEAN, std=VG_STD)
        raw = [imgs, objs, boxes, p.rel, None, None, None, i64_dev[4 * B:5 * B]]
        return packed_batch(self.args, self.trainer, raw, self.dev, counts=p.counts)


def build_vg_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory or its
    split file is not found.  Each path is the flag's value when that exists (--vg_image_dir, --train_h5 / --val_h5,
    --vocab_json), else the reference's layout under --dataroot (sg2im/data/dataset_params.py:40-60): <dataroot>/vg/images,
    /train.h5 or /val.h5, /vocab.json; the split file is taken with either extension, .npz or .h5.  max_objects = 100 and
    min_objects = 16 as there, unless --max_objects / --min_objects say otherwise."""
    base = os.path.join(args.dataroot, "vg")
    image_dir = args.vg_image_dir if args.vg_image_dir and os.path.isdir(args.vg_image_dir) else os.path.join(base, "images")
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
