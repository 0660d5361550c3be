"""CLEVR, the unpacked dataset: a folder of renders and the scenes file, with the input stage on the device (reference:
sg2im/data/clevr_dialog.py, CLEVRDialogDataset).

The reference's clevr_dialog.py shares with its packed_clevr_dialog.py the box formula (:21-77, the same statements), the
scenes file, the dialog file that names the pictures and the four attribute tables.  So `CLEVRDialogDataset` is
`PackedClevrDataset` — its files, `open`, `max_samples`, the object rows and `ClevrBatchBuilder`'s 4-byte pixels and
`ops.clevr_boxes` — with what differs in the reference:

VOCABULARY (:94-122).  Six predicates: `__in_image__` 0, `right` 1, `behind` 2, `front` 3, `left` 4, `__padding__` 5; no
location predicate.  `pred_idx_to_name` is a list here, as for the other datasets of this package.
GRAPH (extract_triplets, :289-307).  The edges are the RENDERER's `relationships`, not relations derived from the boxes:
per key of the scene's `relationships`, then per o1 ascending, a row [o2, pred, o1] for every o2 listed.  Each key's rows are
reduced to their minimal graph (scripts/graphs_utils.py:74-82), or with `--use_transitivity 1` kept whole beside it; the
`__in_image__` dummies follow.  No add_learnt_triplets: no converse draws and no extras, `triplet_type` is ORIGINAL_EDGE
and `conv_counts` zeros.  The rows are listed on the host (`annotations`, which checks their indices) and go up with the
batch's other fields in the one copy of the second staging buffer; the graph is built by `clevr_triplets`, one block per
sample on the device (csrc/clevr_graph.hip).  A sample is at most 64 graph rows with its `__image__` row: a scenes file with
a scene of more than 63 objects is refused when the dataset is made (CLEVR renders at most 10).
COLLATE (:176-179, clevr_collate_fn_fix :387-463).  The `__image__` row follows a sample's objects with the box
(0, 0, 1, 1); padded rows are -1 boxes and zero attributes (collate.packed_batch).
FILTER (:192-199).  `dense_scenes` keeps the scenes of MORE than max_objects objects; there is no other filter.
FLAGS.  `use_transitivity` is 0 or 1 (`clevr_triplets` says why no draw is made for them); any other value is refused.  The
reference's class accepts and ignores learned_transitivity, learned_converse and use_converse — its graph has no such step;
here they are refused, with `packed_clevr` named as the dataset that has them, rather than trained without effect.
MASKS: the reference returns no masks for this dataset; `mask_size` must be 0."""
import os

import numpy as np

from .packed_clevr import ClevrBatchBuilder, PackedClevrDataset, clevr_vocab, split_image_dir  # noqa: F401  (looked_for)

PREDICATES = ("__in_image__", "right", "behind", "front", "left", "__padding__")      # clevr_dialog.py:96-97, by id
CLEVR_MAX_OBJECTS = 10                                     # clevr_dialog.py:82: the constructor's default
ROW_LIMIT = 64                                             # csg_clevr_graph_*: rows per sample, the __image__ row included

_ONLY_PACKED = ("CLEVRDialogDataset: %s is not part of the `clevr` dataset's graph (sg2im/data/clevr_dialog.py:289-307 has no "
                "add_learnt_triplets and no converse relation); `--dataset packed_clevr` is the CLEVR dataset that has it")
_NO_MASKS = ("CLEVRDialogDataset: mask_size must be 0 (got %d): the reference returns no masks for this dataset; "
             "`--dataset packed_clevr` has none either")


class CLEVRDialogDataset(PackedClevrDataset):
    def __init__(self, scenes_json, image_dir, max_objects=CLEVR_MAX_OBJECTS, include_relationships=True, use_transitivity=0,
                 use_converse=False, learned_transitivity=False, learned_converse=False, **kw):
        for name, value in (("learned_transitivity", learned_transitivity), ("learned_converse", learned_converse),
                            ("use_converse", use_converse)):
            if value:
                raise ValueError(_ONLY_PACKED % name)
        if use_transitivity not in (0, 1):
            raise ValueError("CLEVRDialogDataset: use_transitivity must be 0 or 1 (got %r): between them the reference's graph "
                             "depends on its uniform draws (scripts/graphs_utils.py:79-80)" % (use_transitivity,))
        self.use_transitivity = int(use_transitivity)
        self.include_relationships = bool(include_relationships)
        self.max_objects = int(max_objects)
        super().__init__(scenes_json, image_dir, min_objects=0, max_objects=self.max_objects, **kw)
        most = max([len(s["objects"]) for s in self.scenes] + [0])
        if most > ROW_LIMIT - 1:
            raise ValueError("CLEVRDialogDataset: a scene has %d objects, at most %d: a sample has the __image__ row besides, and "
                             "its graph is built in the 64-row kernel (one lane of a wave per row)" % (most, ROW_LIMIT - 1))

    def check_flags(self, mask_size):
        if mask_size:
            raise NotImplementedError(_NO_MASKS % mask_size)

    def make_vocab(self):
        return clevr_vocab(PREDICATES)

    def is_dense(self, n, min_objects, max_objects):
        return n > max_objects                             # clevr_dialog.py:192-199

    def annotations(self, index):
        """PackedClevrDataset.annotations and the scene's relation rows: int64 (R,3) = [o2, pred, o1] in the order
        extract_triplets lists them (clevr_dialog.py:293-297), duplicates kept.  A key that is no predicate of the
        vocabulary, a per-object list that is missing and an index outside the scene's objects are refused here."""
        objs, geom, rot = super().annotations(index)
        scene = self.scenes[index]
        n = objs.shape[0]
        p2i = self.vocab["pred_name_to_idx"]
        rows = []
        for key, lists in scene.get("relationships", {}).items():
            if key not in p2i or key == "__padding__":
                raise ValueError("scene %d: the relationship %r is no predicate of the vocabulary (%s)" % (
                    index, key, ", ".join(PREDICATES[1:5])))
            if len(lists) < n:
                raise ValueError("scene %d: relationships[%r] has %d lists for %d objects" % (index, key, len(lists), n))
            for o1 in range(n):
                for o2 in lists[o1]:
                    if not (isinstance(o2, int) and 0 <= o2 < n):
                        raise ValueError("scene %d: relationships[%r][%d] names object %r outside [0, %d)" % (
                            index, key, o1, o2, n))
                    rows.append((o2, p2i[key], o1))
        return objs, geom, rot, np.asarray(rows, np.int64).reshape(-1, 3)


class ClevrDialogBatchBuilder(ClevrBatchBuilder):
    """ClevrBatchBuilder whose relation rows are a field of the second staging buffer, padded with `__padding__` rows: they
    reach collate.packed_batch as the device view and the host copy, with the objects per sample on the device and on the
    host."""

    def rows(self, indices, sizes, drawn):
        ann = [self.ds.annotations(i) for i in indices]
        fields = self.fields_of(ann)
        rel = np.zeros((len(ann), max(a[3].shape[0] for a in ann), 3), np.int64)
        rel[..., 1] = self.ds.vocab["pred_name_to_idx"]["__padding__"]
        for b, a in enumerate(ann):
            rel[b, :a[3].shape[0]] = a[3]
        fields["rel"] = rel
        return fields, {}

    def assemble(self, dev, p):
        objs, boxes, _, _ = super().assemble(dev, p)
        return objs, boxes, (dev["rel"], p.rel, dev["counts"]), p.counts


CLEVRDialogDataset.builder_class = ClevrDialogBatchBuilder


def build_clevr_dialog_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory does not
    exist.  The paths and their flags are `packed_clevr`'s (sg2im/data/dataset_params.py:24-39 names the same folder):
    base = <dataroot>/CLEVR/CLEVR_Dialog, scenes base/scenes/CLEVR_<split>_scenes.json, pictures base/images/<entry's
    split>/<file name>, dialog file base/clevr_dialog_<split>_raw.json when present; --clevr_<split>_scenes_json and
    --clevr_<split>_image_dir name others.  --max_objects (10 unless given) is read by --dense_scenes alone."""
    base = os.path.join(args.dataroot, "CLEVR", "CLEVR_Dialog")
    given = getattr(args, "clevr_%s_image_dir" % split)
    image_dir = split_image_dir(args, split)
    if not os.path.isdir(image_dir):
        return None
    scenes = getattr(args, "clevr_%s_scenes_json" % split) or os.path.join(base, "scenes", "CLEVR_%s_scenes.json" % split)
    return CLEVRDialogDataset(
        scenes, given or os.path.join(base, "images"), dialog_json=os.path.join(base, "clevr_dialog_%s_raw.json" % split),
        split_dirs=not given, image_size=args.image_size, mask_size=args.mask_size,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        dense_scenes=bool(args.dense_scenes), max_objects=args.max_objects or CLEVR_MAX_OBJECTS,
        include_relationships=bool(args.include_relationships), use_transitivity=args.use_transitivity,
        use_converse=bool(args.use_converse), learned_transitivity=bool(args.learned_transitivity),
        learned_converse=bool(args.learned_converse))
