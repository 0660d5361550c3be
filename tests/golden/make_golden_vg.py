#!/usr/bin/env python3
"""Generate tests/golden/vg_samples.npz by running the REAL reference's packed Visual Genome loader on the CPU:
PackedVGSceneGraphDataset.__getitem__ (sg2im/data/packed_vg.py:67-144) for every sample in order, then vg_collate_fn
(:147-229), on small seeded tables and pictures of recorded sizes.

The constructor needs h5py and torchvision, which make_golden's import shim only stubs; so the object is made with __new__
and its attributes are set by hand: `data` as IntTensors (what :50 makes of the HDF5 arrays), image_paths, image_dir, the
vocabulary, the flags, and a transform that returns zeros (the pictures' pixels are not this file's business, their sizes
are).  The object sampling draws from Python's GLOBAL `random` stream, seeded per setting; a set of small ints and
random.sample are reproducible on one interpreter version, which the metadata records.
Needs the reference checkout (build container only); the output is plain tensors + JSON metadata.
Usage:  python tests/golden/make_golden_vg.py
"""
import os
import platform
import random
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (the reference import shim, save / npy)

from canonicalsg2im_amd.synth import make_vocab  # noqa: E402  (ours: inputs only)

N, MO, MR = 4, 24, 16
OBJECTS_PER_IMAGE = (5, 12, 24, 9)
RELATIONSHIPS_PER_IMAGE = (3, 16, 7, 0)
SIZES = ((333, 500), (481, 640), (200, 201), (1024, 683))          # (HH, WW): no power of two, the quotients are inexact
IMAGE_IDS = (100, 101, 2317, 7)
# (max_objects, use_orphaned_objects, include_relationships, learned_transitivity, seed of the `random` module)
SETTINGS = (
    (100, 1, 1, 0, 7),
    (10, 1, 1, 0, 8),            # samples 1 and 2 keep max_objects of their related objects: 11 rows with __image__
    (100, 0, 1, 0, 9),           # samples 0 .. 2 only: sample 3 has no relationship, so no object at all without the orphans,
                                 # and the reference's add_location_triplets fails on a sample without objects
    (100, 1, 0, 0, 10),
    (100, 1, 1, 1, 7),
    (10, 1, 1, 1, 8),
)


def make_tables(vocab, seed=1):
    rng = np.random.default_rng(seed)
    names = np.full((N, MO), -1, np.int32)
    boxes = np.full((N, MO, 4), -1, np.int32)
    for i, n in enumerate(OBJECTS_PER_IMAGE):
        h, w = SIZES[i]
        names[i, :n] = rng.integers(1, len(vocab["object_idx_to_name"]), n)
        boxes[i, :n] = np.stack([rng.integers(0, w - 40, n), rng.integers(0, h - 40, n), rng.integers(32, w, n),
                                 rng.integers(32, h, n)], 1)
        boxes[i, 0, 0] = 0                                       # x = 0
        boxes[i, 1, 2] = w                                       # w = WW
        boxes[i, 2] = (w - 10, h - 7, 45, 33)                    # runs past the right and the lower edge
    subjects = np.full((N, MR), -1, np.int32)
    predicates, objects = subjects.copy(), subjects.copy()
    plain = [i for i, name in enumerate(vocab["pred_idx_to_name"]) if not name.startswith("__")]
    for i, (n, r) in enumerate(zip(OBJECTS_PER_IMAGE, RELATIONSHIPS_PER_IMAGE)):
        subjects[i, :r] = rng.integers(0, n, r)
        objects[i, :r] = rng.integers(0, n, r)
        predicates[i, :r] = rng.choice(plain, r)
    return {"object_names": names, "object_boxes": boxes, "objects_per_image": np.asarray(OBJECTS_PER_IMAGE, np.int32),
            "relationship_subjects": subjects, "relationship_predicates": predicates, "relationship_objects": objects,
            "relationships_per_image": np.asarray(RELATIONSHIPS_PER_IMAGE, np.int32)}


def fx_vg_samples():
    from PIL import Image
    from sg2im.data.packed_vg import PackedVGSceneGraphDataset, vg_collate_fn
    vocab = make_vocab("vg")
    tables = make_tables(vocab)
    paths = ["VG_100K/%d.png" % i for i in IMAGE_IDS]
    arrays = dict(tables)
    arrays["sizes"] = np.asarray(SIZES, np.int64)
    settings = []
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "VG_100K"))
        for p, (h, w) in zip(paths, SIZES):
            Image.fromarray(np.zeros((h, w, 3), np.uint8), "RGB").save(os.path.join(tmp, p))
        for si, (max_objects, orphans, rels, trans, seed) in enumerate(SETTINGS):
            ds = PackedVGSceneGraphDataset.__new__(PackedVGSceneGraphDataset)
            ds.include_dummies, ds.learned_transitivity, ds.learned_converse, ds.learned_symmetry = True, bool(trans), False, False
            ds.image_dir, ds.image_size, ds.image_paths, ds.vocab = tmp, (64, 64), paths, vocab
            ds.max_objects, ds.use_orphaned_objects, ds.include_relationships = max_objects, bool(orphans), bool(rels)
            ds.transform = lambda im: torch.zeros(3, 4, 4)
            ds.data = {k: torch.IntTensor(v) for k, v in tables.items()}
            random.seed(seed)
            which = [i for i in range(N) if orphans or RELATIONSHIPS_PER_IMAGE[i]]
            samples = [ds[i] for i in which]
            _, objs, boxes, triplets, _, ttype, masks, ids = vg_collate_fn(vocab, samples)
            assert masks is None and ids.tolist() == [IMAGE_IDS[i] for i in which]
            tag = "s%d_" % si
            arrays.update({tag + "objs": mg.npy(objs[:, :, 0]).astype(np.int16), tag + "boxes": mg.npy(boxes),
                           tag + "n": np.asarray([s[1]["objects"].numel() for s in samples], np.int64),
                           tag + "triplets": mg.npy(triplets).astype(np.int16), tag + "tt": mg.npy(ttype).astype(np.int8)})
            settings.append({"max_objects": max_objects, "use_orphaned_objects": orphans, "include_relationships": rels,
                             "learned_transitivity": trans, "learned_converse": 0, "seed": seed, "samples": which,
                             "objects": list(objs.shape), "triplets": list(triplets.shape)})
    assert boxes.dtype == torch.float32
    mg.save("vg_samples", {"ref": "sg2im/data/packed_vg.py:67-144 (__getitem__), :147-229 (vg_collate_fn); "
                                  "sg2im/data/base_dataset.py:35-151",
                           "vocab": "vg", "python": platform.python_version(), "image_paths": paths,
                           "image_ids": list(IMAGE_IDS), "sizes": "(HH, WW) of the decoded pictures", "settings": settings,
                           "dtypes": "objs / triplets int16, tt int8 (int64 in the collate); the tables int32; n = objects "
                                     "per sample with its __image__ row"},
            **arrays)
    for s in settings:
        print(s)


if __name__ == "__main__":
    torch.set_num_threads(4)
    fx_vg_samples()
