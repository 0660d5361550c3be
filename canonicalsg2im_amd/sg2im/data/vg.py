"""Visual Genome, the unpacked dataset: a folder of pictures and a split file, with the input stage on the device (reference:
sg2im/data/vg.py).

The reference's vg.py is its packed_vg.py without `add_location_triplets`: __getitem__'s object choice, the per-object rows
and vg_collate_fn are the same statements (vg.py:86-146 against packed_vg.py:77-137).  So `VGSceneGraphDataset` is
`PackedVGDataset` — its `load_split`, `select`, `load` and `VGBatchBuilder` — with what differs in the reference:

FOLDER (sg2im/data/dataset_params.py:110-127, vg.py:27-29, :49).  One directory, <dataroot>/VisualGenome, holds the split
file, vocab.json and the pictures; `image_paths` are relative to it.
VOCABULARY (vg.py:64-71).  `attributes = {"objects": object_name_to_idx}` with its reverse, and `__padding__` appended as the
last predicate.  No location predicate is registered: the predicate table is vocab.json's plus `__padding__`.
FLAGS.  `use_converse` raises ValueError (vg.py:73-74); `use_transitivity` is accepted and unused, as there.  max_objects is
10 and min_objects 3 unless given (dataset_params.py:114-115).  A sample keeps up to max_objects objects (the reference's
off-by-one, packed_vg.py of this package) and has the `__image__` row besides; its graph is built by csg_canon_small_*, which
takes 64 rows, so max_objects above 63 is refused when the dataset is made.
GRAPH (vg.py:136-149).  The annotated rows and the `__in_image__` dummies, through `annotated_triplets`: converse draws,
transitive extras, np.unique's order and the collate's padding, one block per sample on the device (csrc/canon_small.hip).
As for every folder dataset of this package the `__image__` row and the dummies are always there (collate.packed_batch
appends the row): `--include_dummies` is not consulted.
MASKS: the reference returns `masks = None` (vg.py:151); `mask_size` must be 0.

The annotated rows go up with the batch's other fields in the one copy of the second staging buffer and stay on the device;
the host keeps its copy for the entry's checks and to count the converse draws."""
import os

import numpy as np

from .packed_vg import PackedVGDataset, VGBatchBuilder, split_file

VG_MAX_OBJECTS, VG_MIN_OBJECTS = 10, 3                     # sg2im/data/dataset_params.py:114-115
VG_ROW_LIMIT = 64                                          # csg_canon_small_*: rows per sample, the __image__ row included

_NO_MASKS = ("VGSceneGraphDataset: mask_size must be 0 (got %d): the reference returns masks = None for this dataset "
             "(sg2im/data/vg.py:151)")
_TOO_MANY = ("VGSceneGraphDataset: max_objects = %d, at most %d: a sample keeps up to max_objects objects and has the "
             "__image__ row besides, and its graph is built in the 64-row kernel (one lane of a wave per row)")


class VGSceneGraphDataset(PackedVGDataset):
    def __init__(self, split_path, image_dir, vocab_json, image_size=(256, 256), max_objects=VG_MAX_OBJECTS, **kw):
        super().__init__(split_path, image_dir, vocab_json, image_size=image_size, max_objects=max_objects, **kw)   # vg.py:17-21

    def check_flags(self, use_transitivity, use_converse, mask_size, max_objects):
        if use_converse:
            raise ValueError("VGSceneGraphDataset: use_converse is not implemented, as in the reference (sg2im/data/vg.py:73-74)")
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)
        if max_objects > VG_ROW_LIMIT - 1:
            raise ValueError(_TOO_MANY % (max_objects, VG_ROW_LIMIT - 1))

    def add_predicates(self):
        self.vocab["pred_name_to_idx"]["__padding__"] = len(self.vocab["pred_name_to_idx"].values())      # vg.py:70-71
        self.vocab["pred_idx_to_name"].append("__padding__")


class VGAnnotatedBatchBuilder(VGBatchBuilder):
    """VGBatchBuilder whose annotated rows are a field of the second staging buffer: they reach collate.packed_batch as the
    device view and the host copy."""

    def rows(self, indices, sizes, picked):
        fields, extras = super().rows(indices, sizes, picked)
        fields["rel"] = np.ascontiguousarray(extras.pop("rel").numpy())
        return fields, extras

    def assemble(self, dev, p):
        objs, boxes, rel_host, counts = super().assemble(dev, p)
        return objs, boxes, (dev["rel"], rel_host), counts


VGSceneGraphDataset.builder_class = VGAnnotatedBatchBuilder


def _base(args):
    return os.path.join(args.dataroot, "VisualGenome")


def split_image_dir(args, split):
    """Where the pictures are looked for: --vg_image_dir when it exists, else <dataroot>/VisualGenome (every split's)."""
    return args.vg_image_dir if args.vg_image_dir and os.path.isdir(args.vg_image_dir) else _base(args)


def split_path(args, split):
    """The split file as the command line names it: --train_h5 / --val_h5 when it exists (with either extension), else
    <dataroot>/VisualGenome/<split>.h5."""
    given = getattr(args, "%s_h5" % split)
    return given if split_file(given) else os.path.join(_base(args), "%s.h5" % split)


def build_vg_unpacked_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory or its
    split file is not found.  Each path is the flag's value when that exists (--vg_image_dir, --train_h5 / --val_h5,
    --vocab_json), else the reference's layout (sg2im/data/dataset_params.py:110-127): <dataroot>/VisualGenome holds the
    pictures, train.h5 or val.h5 and vocab.json; the split file is taken with either extension, .npz or .h5.  max_objects =
    10 and min_objects = 3 as there, unless --max_objects / --min_objects say otherwise."""
    image_dir = split_image_dir(args, split)
    found = split_file(split_path(args, split))
    if not os.path.isdir(image_dir) or found is None:
        return None
    vocab_json = args.vocab_json if args.vocab_json and os.path.isfile(args.vocab_json) else os.path.join(_base(args), "vocab.json")
    return VGSceneGraphDataset(
        found, image_dir, vocab_json, image_size=args.image_size, mask_size=args.mask_size,
        min_objects=args.min_objects or VG_MIN_OBJECTS, max_objects=args.max_objects or VG_MAX_OBJECTS,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        include_relationships=bool(args.include_relationships), use_orphaned_objects=bool(args.vg_use_orphaned_objects),
        use_transitivity=bool(args.use_transitivity), use_converse=bool(args.use_converse))
