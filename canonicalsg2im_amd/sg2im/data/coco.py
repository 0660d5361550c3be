"""COCO / COCO-Stuff with the original sg2im graph: every object draws one partner (reference: sg2im/data/coco.py).

`--dataset coco`, the trainer's default.  `CocoSceneGraphDataset` is `PackedCocoSceneGraphDataset` (packed_coco.py of this
package: the two annotation files, the reference's filtering rules :162-277, the vocabulary) at the reference's limits for
this dataset (sg2im/data/dataset_params.py:128-141): 3 to 8 objects unless --min_objects / --max_objects say otherwise.

What differs is the GRAPH (:365-428).  packed_coco relates all pairs by their geometry and reduces per relation.  Here every
real object `cur` draws ONE other object of its picture and a coin from Python's `random`, and the pair gets one predicate:
__surrounding__ / __inside__ from the boxes, otherwise the quadrant of the centre difference; with `use_converse` inside,
right of and below become surrounding, left of and above with subject and object swapped.  Then the __in_image__ dummies
and add_learnt_triplets, as for every dataset.

Who does what.  The draws are made on the host, in batch order, on the consumer's thread (`CocoPairsBatchBuilder.draw`):
the reference's calls in the reference's order, so the same state of `rng` gives the reference's own pairs on one
interpreter version.  They travel with the category ids, the boxes and the counts in the second staging buffer.  The
predicates (`ops.pair_relations`), the `__image__` row and the canonical graph over the sampled rows
(csg_canon_general_build_dev, then the converse / close / emit entries packed_vg uses) run on the device, as do Pillow's
resize, ToTensor and the ImageNet Normalize (`ops.preprocess_images`).

MASKS ARE OPT-IN, as for packed_coco (its docstring has the whole of it): without `segmentations=True`
(`--coco_segmentations 1`) `mask_size` must be 0 and object centres are BOX centres, x0 + 0.5 * w — the reference takes the
centroid of the decoded mask and falls back to exactly this expression when a mask is empty (:356-358).  With it the
segmentations are decoded on the device (`ops.coco_masks`), the batch carries the masks, and the mask centroids are the
centres `ops.pair_relations` compares; with mask_size == 0 they are decoded at the reference's working size for this dataset,
32 (:152-154), for the centres alone.  Equality with pycocotools' and OpenCV's output has not been run.

LIMIT: at most 255 objects per picture.  The canonical graph takes 256 rows per sample, one of which is `__image__`; an
image that passes the filters with more objects is refused when the dataset is made (`--max_objects 1000`, the README's
command line, is served up to that).

VALIDATION SPLIT.  The reference's `val` is val2017 intersected with a list of image ids written into its source.  That list
is not part of this package: `--coco_val_ids FILE` names a JSON list of ids and `val` keeps the images on it, in annotation
order; without the flag `val` is all of val2017."""
import json
import os
import random

import numpy as np

from .loader import BatchBuilder
from .packed_coco import _NO_MASKS, PackedCocoSceneGraphDataset, device_masks, segmentation_fields, split_image_dir

COCO_MIN_OBJECTS, COCO_MAX_OBJECTS = 3, 8                  # sg2im/data/dataset_params.py:132-133
MAX_OBJECTS_PER_PICTURE = 255                              # csg_canon_general_*: 256 rows with __image__

_TOO_MANY = ("CocoSceneGraphDataset: image %s keeps %d objects; the canonical graph takes at most %d per picture (256 rows "
             "with __image__): lower --max_objects or raise --min_object_size")


class CocoSceneGraphDataset(PackedCocoSceneGraphDataset):
    default_mask_size = 32                                 # what the reference decodes at with mask_size == 0 (:152-154)

    def __init__(self, image_dir, instances_json, stuff_json, image_size=(64, 64), mask_size=0, normalize_images=True,
                 max_samples=None, include_relationships=True, min_object_size=0.02, min_objects=COCO_MIN_OBJECTS,
                 max_objects=COCO_MAX_OBJECTS, include_other=False, instance_whitelist=None, stuff_whitelist=None,
                 use_converse=False, keep_image_ids=None, segmentations=False):
        super().__init__(image_dir, instances_json, stuff_json, image_size=image_size, mask_size=mask_size,
                         normalize_images=normalize_images, max_samples=max_samples, min_object_size=min_object_size,
                         min_objects=min_objects, max_objects=max_objects, include_other=include_other,
                         instance_whitelist=instance_whitelist, stuff_whitelist=stuff_whitelist, segmentations=segmentations)
        self.include_relationships = bool(include_relationships)
        self.use_converse = bool(use_converse)
        if keep_image_ids is not None:                     # dataset_params.py:187-189, in annotation order
            keep = set(int(i) for i in keep_image_ids)
            self.image_ids = [i for i in self.image_ids if i in keep]
        for i in self.image_ids:
            if len(self.image_id_to_objects[i]) > MAX_OBJECTS_PER_PICTURE:
                raise ValueError(_TOO_MANY % (i, len(self.image_id_to_objects[i]), MAX_OBJECTS_PER_PICTURE))

    def num_objects(self, index):
        return len(self.image_id_to_objects[self.image_ids[index]])


def draw_pairs(n, rng=random, include_relationships=True):
    """The draws of one sample with `n` real objects (coco.py:372-380), in the reference's order: for every object `cur`
    one `choice` among the others, then one `random` -> [(other, flip)], flip = the pair is (other, cur).  Nothing is drawn
    for fewer than two objects or without relationships (:374-375)."""
    pairs = []
    if n >= 2 and include_relationships:
        for cur in range(n):
            other = rng.choice([j for j in range(n) if j != cur])
            flip = not (rng.random() > 0.5)
            pairs.append((other, flip))
    return pairs


class CocoPairsBatchBuilder(BatchBuilder):
    """Batches of a CocoSceneGraphDataset (loader.BatchBuilder has the two halves of a batch): every picture goes up as RGB,
    ImageNet normalisation.  Before anything else start() calls `draw_pairs` for every sample in batch order on the
    consumer's thread (the order decides what the random stream gives whom, so the workers do not do it).  The fields of
    its own are the category ids, the boxes over the decoded sizes, the counts, and the draws: other int32 (B,O), -1 where
    nothing was drawn, flip uint8 (B,O).  No kernel of its own runs in assemble: the pairs reach collate.packed_batch in
    the batch's triplet slot, as device views with their host copies.  A dataset that reads segmentations adds their fields,
    and assemble launches ops.coco_masks (packed_coco.device_masks).

    `rng`: where the draws come from; by default a random.Random of the builder's own, seeded from (0, rank).  A resumed
    run starts it afresh: its epoch order is the interrupted run's, its pairs are not."""

    takes_rng = True

    def __init__(self, dataset, args, trainer, device, num_workers=1, rng=None):
        super().__init__(dataset, args, trainer, device, num_workers=num_workers)
        if rng is None:
            from ... import dist
            rng = random.Random((0 << 32) | dist.rank())
        self.rng = rng

    def draw(self, indices):
        counts = [self.ds.num_objects(i) for i in indices]
        if max(counts) < 1:
            raise ValueError("a batch of samples without objects")
        return [draw_pairs(n, self.rng, self.ds.include_relationships) for n in counts]      # in batch order

    def rows(self, indices, sizes, drawn):
        ann = [self.ds.annotations(i, w, h) for i, (h, w) in zip(indices, sizes.tolist())]
        B, O = len(ann), max(a[0].shape[0] for a in ann)
        objs = np.zeros((B, O, 1), np.int64)
        boxes = np.full((B, O, 4), -1.0, np.float32)
        other = np.full((B, O), -1, np.int32)
        flip = np.zeros((B, O), np.uint8)
        for b, ((o, bx), pairs) in enumerate(zip(ann, drawn)):
            objs[b, :o.shape[0], 0] = o
            boxes[b, :bx.shape[0]] = bx
            if pairs:
                other[b, :len(pairs)] = [j for j, _ in pairs]
                flip[b, :len(pairs)] = [f for _, f in pairs]
        seg = segmentation_fields(self, indices, sizes, O) if self.ds.segmentations else {}
        return {"objs": objs, "boxes": boxes, "counts": np.asarray([a[0].shape[0] for a in ann], np.int64), "other": other,
                "flip": flip, **seg}, {}

    def assemble(self, dev, p):
        pairs = (dev["other"], dev["flip"], p.other, p.flip) if self.ds.include_relationships else None
        if self.ds.segmentations:
            return dev["objs"], dev["boxes"], pairs, p.counts, device_masks(self.ds, dev, p)
        return dev["objs"], dev["boxes"], pairs, p.counts


CocoSceneGraphDataset.builder_class = CocoPairsBatchBuilder


def build_coco_pairs_dataset(args, split):
    """The folder dataset of `split` ("train" / "val") named by the command line, or None when its image directory does not
    exist.  Paths as packed_coco's build_coco_dataset: --coco_<split>_image_dir / _instances_json / _stuff_json, by default
    the reference's layout under --dataroot (sg2im/data/dataset_params.py:142-152).  `val` with --coco_val_ids: the images
    of val2017 whose ids are on that JSON list."""
    root = os.path.join(args.dataroot, "MSCoco")
    image_dir = split_image_dir(args, split)
    if not os.path.isdir(image_dir):
        return None
    segmentations = bool(getattr(args, "coco_segmentations", 0))
    if args.mask_size and not segmentations:
        raise NotImplementedError(_NO_MASKS % args.mask_size)
    inst = getattr(args, "coco_%s_instances_json" % split) or os.path.join(root, "annotations", "instances_%s2017.json" % split)
    stuff = getattr(args, "coco_%s_stuff_json" % split) or os.path.join(root, "annotations", "stuff_%s2017.json" % split)
    keep = None
    if split == "val" and getattr(args, "coco_val_ids", None):
        with open(args.coco_val_ids, "r") as f:
            keep = json.load(f)
        if not isinstance(keep, list) or not all(isinstance(i, int) and not isinstance(i, bool) for i in keep):
            raise ValueError("--coco_val_ids %s: a JSON list of image ids is expected" % args.coco_val_ids)
    return CocoSceneGraphDataset(
        image_dir, inst, stuff, image_size=args.image_size, mask_size=args.mask_size,
        max_samples=args.num_train_samples if split == "train" else args.num_val_samples,
        include_relationships=bool(args.include_relationships), min_object_size=args.min_object_size,
        min_objects=args.min_objects or COCO_MIN_OBJECTS, max_objects=args.max_objects or COCO_MAX_OBJECTS,
        use_converse=bool(args.use_converse), keep_image_ids=keep, segmentations=segmentations)
