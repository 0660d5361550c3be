#!/usr/bin/env python3
"""Generate tests/golden/vg_unpacked.npz by running the REAL reference's unpacked Visual Genome loader on the CPU:
VGSceneGraphDataset.__getitem__ (sg2im/data/vg.py:76-151) for every sample in order, then vg_collate_fn (:154-236), on small
seeded tables and pictures of recorded sizes.

As in make_golden_vg.py the object is made with __new__ and its attributes are set by hand (the constructor needs h5py and
torchvision, which make_golden's import shim only stubs): `data` as IntTensors, image_paths, image_dir, the flags, a transform
that returns zeros, and the vocabulary as the constructor leaves it (:64-71) from a small vocab.json-shaped dict WITHOUT
location predicates, which the metadata records.  The object sampling draws from Python's GLOBAL `random` stream, seeded per
setting (reproducible on one interpreter version, which the metadata records); with learned_converse the draws come from
numpy's GLOBAL stream, seeded per setting, as make_golden_annotated.py does.
Needs the reference checkout (build container only); the output is plain tensors + JSON metadata.
Usage:  python tests/golden/make_golden_vg_unpacked.py
"""
import copy
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

N, MO, MR = 4, 24, 20
OBJECTS_PER_IMAGE = (5, 12, 24, 9)
RELATIONSHIPS_PER_IMAGE = (3, 20, 9, 0)
SIZES = ((333, 500), (481, 640), (200, 201), (1024, 683))          # (HH, WW): no power of two, the quotients are inexact
IMAGE_IDS = (100, 101, 2317, 7)
# (max_objects, use_orphaned_objects, include_relationships, learned_transitivity, learned_converse, seed of `random` and,
# with learned_converse, of numpy's global stream)
SETTINGS = (
    (30, 1, 1, 0, 0, 7),
    (10, 1, 1, 0, 0, 8),         # sample 2 keeps max_objects of its related objects: 11 rows with __image__
    (30, 0, 1, 0, 0, 9),         # samples 0 .. 2 only: sample 3 has no relationship, so no object at all without the orphans,
                                 # and the reference's add_learnt_triplets fails on a sample without a row
    (30, 1, 0, 0, 0, 10),        # the dummies alone
    (30, 1, 1, 1, 0, 7),
    (10, 1, 1, 1, 0, 8),
    (10, 0, 1, 1, 0, 11),
    (30, 1, 0, 1, 0, 10),
    (30, 1, 1, 1, 1, 12),
    (10, 1, 1, 0, 1, 13),
)


def vocab_json():
    """A vocab.json as scripts/preprocess_vg.py leaves it: `__image__` is object 0, `__in_image__` predicate 0, then the
    annotated predicates; no `__padding__` and no location predicate."""
    v = make_vocab("vg")
    preds = ["__in_image__"] + [p for p in v["pred_idx_to_name"] if not p.startswith("__")]
    return {"object_name_to_idx": dict(v["object_name_to_idx"]), "object_idx_to_name": list(v["object_idx_to_name"]),
            "pred_name_to_idx": {p: i for i, p in enumerate(preds)}, "pred_idx_to_name": preds}


def constructed(vocab):
    """vg.py:64-71 on a copy."""
    vocab = copy.deepcopy(vocab)
    vocab["attributes"] = {"objects": vocab["object_name_to_idx"]}
    vocab["reverse_attributes"] = {a: {v: k for k, v in t.items()} for a, t in vocab["attributes"].items()}
    vocab["pred_name_to_idx"]["__padding__"] = len(vocab["pred_name_to_idx"].values())
    vocab["pred_idx_to_name"].append("__padding__")
    return vocab


def make_tables(vocab, seed=21):
    rng = np.random.default_rng(seed)
    names = np.full((N, MO), -1, np.int32)
    boxes = np.full((N, MO, 4), -1, np.int32)
    for i, n in enumerate(OBJECTS_PER_IMAGE):
        h, w = SIZES[i]
        names[i, :n] = rng.integers(1, len(vocab["object_idx_to_name"]), n)
        boxes[i, :n] = np.stack([rng.integers(0, w - 40, n), rng.integers(0, h - 40, n), rng.integers(32, w, n),
                                 rng.integers(32, h, n)], 1)
    subjects = np.full((N, MR), -1, np.int32)
    predicates, objects = subjects.copy(), subjects.copy()
    plain = [i for i, name in enumerate(vocab["pred_idx_to_name"]) if not name.startswith("__")]
    few = (plain[0], plain[3], plain[-1])                        # few predicates: chains, cycles and converse hits happen
    for i, (n, r) in enumerate(zip(OBJECTS_PER_IMAGE, RELATIONSHIPS_PER_IMAGE)):
        subjects[i, :r] = rng.integers(0, n, r)
        objects[i, :r] = rng.integers(0, n, r)
        predicates[i, :r] = rng.choice(few if i == 1 else plain, r)
    # sample 1: a chain 0 -> 1 -> 2 -> 3 and a cycle 4 -> 5 -> 4 of one predicate, a duplicated row, a self-relation
    subjects[1, :8] = (0, 1, 2, 4, 5, 0, 6, 1)
    objects[1, :8] = (1, 2, 3, 5, 4, 1, 6, 2)
    predicates[1, :8] = (few[0],) * 6 + (few[1], few[0])
    return {"object_names": names, "object_boxes": boxes, "objects_per_image": np.asarray(OBJECTS_PER_IMAGE, np.int32),
            "relationship_subjects": subjects, "relationship_predicates": predicates, "relationship_objects": objects,
            "relationships_per_image": np.asarray(RELATIONSHIPS_PER_IMAGE, np.int32)}


def fx_vg_unpacked():
    from PIL import Image
    from sg2im.data.vg import VGSceneGraphDataset, vg_collate_fn
    on_disk = vocab_json()
    vocab = constructed(on_disk)
    P = len(vocab["pred_idx_to_name"])
    tables = make_tables(vocab)
    paths = ["VG_100K/%d.png" % i for i in IMAGE_IDS]
    arrays = dict(tables)
    arrays["sizes"] = np.asarray(SIZES, np.int64)
    wrng = np.random.default_rng(77)
    settings = []
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "VG_100K"))
        for p, (h, w) in zip(paths, SIZES):
            Image.fromarray(np.zeros((h, w, 3), np.uint8), "RGB").save(os.path.join(tmp, p))
        for si, (max_objects, orphans, rels, trans, conv, seed) in enumerate(SETTINGS):
            ds = VGSceneGraphDataset.__new__(VGSceneGraphDataset)
            ds.include_dummies, ds.learned_transitivity, ds.learned_converse, ds.learned_symmetry = True, bool(trans), bool(conv), False
            ds.image_dir, ds.image_size, ds.image_paths, ds.vocab = tmp, (64, 64), paths, vocab
            ds.max_objects, ds.use_orphaned_objects, ds.include_relationships = max_objects, bool(orphans), bool(rels)
            ds.transform = lambda im: torch.zeros(3, 4, 4)
            ds.data = {k: torch.IntTensor(v) for k, v in tables.items()}
            tag = "s%d_" % si
            if conv:
                w = torch.from_numpy(wrng.normal(size=(P, P)).astype(np.float32))
                up = torch.triu(w, diagonal=0)
                ds.converse_candidates_weights = (up + up.t()).detach().cpu().numpy()      # model.py:10-13, train.py:276
                arrays[tag + "weights"] = ds.converse_candidates_weights.copy()
            random.seed(seed)
            np.random.seed(seed)
            which = [i for i in range(N) if orphans or RELATIONSHIPS_PER_IMAGE[i]]
            samples = [ds[i] for i in which]
            _, objs, boxes, triplets, conv_counts, ttype, masks, ids = vg_collate_fn(vocab, samples)
            assert masks is None and ids.tolist() == [IMAGE_IDS[i] for i in which]
            assert conv_counts.dtype == torch.float32 and tuple(conv_counts.shape) == (len(which), P, P + 1)
            arrays.update({tag + "objs": mg.npy(objs[:, :, 0]).astype(np.int16), tag + "boxes": mg.npy(boxes),
                           tag + "n": np.asarray([s[1]["objects"].numel() for s in samples], np.int64),
                           tag + "counts": np.asarray([len(s[3]) for s in samples], np.int64),
                           tag + "triplets": mg.npy(triplets).astype(np.int16), tag + "tt": mg.npy(ttype).astype(np.int8)})
            draws = int(conv_counts.sum())
            assert bool(draws) == bool(conv and rels)
            if conv:
                nz = mg.npy(conv_counts).reshape(len(which) * P, P + 1)   # conv_counts: mostly zero rows, stored sparse
                rows = np.nonzero(nz.any(axis=1))[0]
                arrays.update({tag + "conv_rows": rows.astype(np.int32), tag + "conv_vals": nz[rows].astype(np.float32)})
            settings.append({"max_objects": max_objects, "use_orphaned_objects": orphans, "include_relationships": rels,
                             "learned_transitivity": trans, "learned_converse": conv, "seed": seed, "draws": draws,
                             "samples": which, "objects": list(objs.shape), "triplets": list(triplets.shape),
                             "extras": int((ttype == 1).sum())})
    assert boxes.dtype == torch.float32
    mg.save("vg_unpacked", {"ref": "sg2im/data/vg.py:76-151 (__getitem__), :154-236 (vg_collate_fn); "
                                   "sg2im/data/base_dataset.py:89-151; scripts/graphs_utils.py:15-27,101-105,130-155",
                            "vocab_json": on_disk, "python": platform.python_version(), "image_paths": paths,
                            "image_ids": list(IMAGE_IDS), "sizes": "(HH, WW) of the decoded pictures", "settings": settings,
                            "dtypes": "objs / triplets int16, tt int8 (int64 in the collate); the tables int32; n = objects "
                                      "per sample with its __image__ row; counts = triplets per sample; conv_counts "
                                      "(B,P,P+1) float32 as the rows of its (B*P, P+1) view that hold a draw; with "
                                      "learned_converse numpy's global stream is seeded with `seed` before the first sample"},
            **arrays)
    for s in settings:
        print(s)


if __name__ == "__main__":
    torch.set_num_threads(4)
    fx_vg_unpacked()
