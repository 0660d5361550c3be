#!/usr/bin/env python3
"""Generate tests/golden/coco_pairs.npz by running the REAL reference's unpacked COCO loader on the CPU:
CocoSceneGraphDataset.__getitem__ (sg2im/data/coco.py:287-430) for every sample of a group in order, then coco_collate_fn
(:452-545), on hand-made annotations and pictures of recorded sizes.

The constructor reads annotation files and needs torchvision, which make_golden's import shim only stubs; so the object is
made with __new__ and its attributes are set by hand: the image ids, file names, per-image annotation rows, the vocabulary
(categories below + BaseDataset.register_augmented_relations), the flags, and a transform that returns zeros (the pictures'
pixels are not this file's business, their sizes are).

SUBSTITUTION.  Decoding a segmentation needs pycocotools and cv2, which are stubs here.  The module's `seg_to_mask` is
patched to return zeros and the stubbed `cv2.resize` to return an (M, M) zero array: every mask is then EMPTY, and the
reference itself takes its fallback centre `x0 + 0.5 * w`, `y0 + 0.5 * h` (:356-358) — the box centre, which is what this
package's datasets use throughout.

The pairs are drawn from Python's GLOBAL `random` stream, seeded per (setting, group); the module's `random` is wrapped only
to RECORD what choice() and random() return.  The learned-converse setting also draws from numpy's global stream, seeded
likewise.  Both are reproducible on one interpreter / numpy version, which the metadata records.
Needs the reference checkout (build container only); the output is plain arrays + JSON metadata.
Usage:  python tests/golden/make_golden_coco.py
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

INSTANCE_CATEGORIES = ((1, "person"), (2, "bicycle"), (3, "car"), (6, "bus"))
STUFF_CATEGORIES = ((92, "banner"), (95, "bridge"), (106, "sky-other"), (183, "other"))
M = 32                                                     # the mask size the reference works at with mask_size == 0

# (image id, (HH, WW), [(category id, x, y, w, h) in pixels]): instances first, then stuff, as the reference lists them
A = 64                                                     # the tie offset in pixels on a 256 x 256 picture: 0.25 exactly


def _tie(image_id, dx, dy):
    return (image_id, (256, 256), [(1, 64, 64, 64, 64), (92, 64 + dx, 64 + dy, 64, 64)])


SAMPLES = [
    # group 0: small pictures of odd sizes, 1, 2, 3, 5 and 8 objects
    (11, (48, 64), [(106, 0, 0, 64, 30)]),
    (12, (37, 53), [(2, 5, 4, 20, 17), (95, 21, 9, 30, 25)]),
    (13, (64, 64), [(1, 3, 8, 30, 40), (3, 30, 20, 33, 21), (106, 0, 0, 64, 22)]),
    (14, (50, 41), [(1, 2, 3, 18, 30), (1, 20, 5, 19, 28), (6, 8, 25, 30, 22), (92, 0, 0, 41, 12), (95, 5, 30, 33, 19)]),
    (15, (33, 64), [(1, 1, 1, 14, 20), (2, 16, 2, 15, 19), (3, 33, 4, 16, 18), (6, 48, 3, 15, 21), (1, 8, 10, 20, 22),
                    (3, 25, 9, 22, 23), (106, 0, 0, 64, 11), (95, 0, 20, 64, 13)]),
    # group 1: two objects, `other` is forced; the centre difference of object 1 - object 0 is an exact tie
    _tie(21, A, A), _tie(22, A, -A), _tie(23, -A, A), _tie(24, -A, -A), _tie(25, 0, -A), _tie(26, -A, 0), _tie(27, 0, A),
    _tie(28, A, 0),
    # group 2: same centre (0, 0): object 0's corners surround object 1, its centre does not exceed object 1's centre;
    # then a pair that surrounds by the reference's own test (x0 < ox0 and the centre beyond the other's centre)
    (31, (256, 256), [(1, 64, 64, 64, 64), (92, 72, 72, 48, 48)]),
    (32, (256, 256), [(3, 0, 0, 200, 200), (106, 10, 10, 100, 100)]),
]
GROUPS = ([0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10, 11, 12], [13, 14])
# (use_converse, learned_transitivity, include_relationships, learned_converse, seed)
SETTINGS = ((0, 0, 1, 0, 3), (1, 0, 1, 0, 4), (0, 1, 1, 0, 5), (1, 1, 1, 0, 6), (0, 0, 0, 0, 7), (0, 1, 1, 1, 8))


class _Recorder:
    """The `random` the reference module sees: the global stream's own answers, written down."""

    def __init__(self):
        self.log = []

    def choice(self, seq):
        r = random.choice(seq)
        self.log.append(["choice", int(r)])
        return r

    def random(self):
        r = random.random()
        self.log.append(["random", r])
        return r


def fx_coco_pairs():
    from PIL import Image
    import sg2im.data.coco as ref
    from sg2im.data.coco import CocoSceneGraphDataset, coco_collate_fn

    ref.seg_to_mask = lambda seg, width=1.0, height=1.0: np.zeros((int(height), int(width)), np.uint8)
    ref.cv2.resize = lambda src, dsize, interpolation=None: np.zeros((dsize[1], dsize[0]))
    ref.cv2.INTER_NEAREST = 0
    rec = _Recorder()
    ref.random = rec

    names = {"object_name_to_idx": {}, "pred_name_to_idx": {}}
    for cid, name in INSTANCE_CATEGORIES + STUFF_CATEGORIES:
        names["object_name_to_idx"][name] = cid
    names["object_name_to_idx"]["__image__"] = 0
    O = max(len(rows) for _, _, rows in SAMPLES)
    cats = np.zeros((len(SAMPLES), O), np.int64)
    boxes_px = np.full((len(SAMPLES), O, 4), -1, np.int64)
    for i, (_, _, rows) in enumerate(SAMPLES):
        cats[i, :len(rows)] = [r[0] for r in rows]
        boxes_px[i, :len(rows)] = [r[1:] for r in rows]
    arrays = {"image_ids": np.asarray([s[0] for s in SAMPLES], np.int64), "sizes": np.asarray([s[1] for s in SAMPLES], np.int64),
              "counts": np.asarray([len(s[2]) for s in SAMPLES], np.int64), "cats": cats, "boxes_px": boxes_px}
    settings, seen = [], set()
    with tempfile.TemporaryDirectory() as tmp:
        for image_id, (h, w), _ in SAMPLES:
            Image.fromarray(np.zeros((h, w, 3), np.uint8), "RGB").save(os.path.join(tmp, "%012d.png" % image_id))
        for si, (conv, trans, rels, lconv, seed) in enumerate(SETTINGS):
            ds = CocoSceneGraphDataset.__new__(CocoSceneGraphDataset)
            ds.vocab = {k: dict(v) for k, v in names.items()}
            ds.register_augmented_relations()
            ds.vocab["attributes"] = {"objects": ds.vocab["object_name_to_idx"]}
            ds.use_converse, ds.learned_transitivity, ds.learned_converse = bool(conv), bool(trans), bool(lconv)
            ds.learned_symmetry, ds.include_dummies, ds.use_transitivity = False, True, False
            ds.include_relationships, ds.masks, ds.mask_size, ds.max_samples = bool(rels), False, M, None
            ds.image_dir, ds.image_size, ds.transform = tmp, (64, 64), (lambda im: torch.zeros(3, 4, 4))
            ds.image_ids = [s[0] for s in SAMPLES]
            ds.image_id_to_filename = {s[0]: "%012d.png" % s[0] for s in SAMPLES}
            ds.image_id_to_objects = {s[0]: [{"category_id": r[0], "bbox": [float(v) for v in r[1:]], "segmentation": []}
                                             for r in s[2]] for s in SAMPLES}
            P = len(ds.vocab["pred_name_to_idx"])
            if lconv:
                w = torch.from_numpy(np.random.default_rng(seed).normal(size=(P, P)).astype(np.float32))
                up = torch.triu(w, diagonal=0)
                ds.converse_candidates_weights = (up + up.t()).detach().cpu().numpy()      # model.py:10-13, train.py:276
                arrays["s%d_weights" % si] = ds.converse_candidates_weights.copy()
            at_dummies = []
            inner = ds.add_dummy_triplets

            def wrapped(objs, triplets, inner=inner, at_dummies=at_dummies):
                at_dummies.append([[int(v) for v in t] for t in triplets])
                return inner(objs, triplets)

            ds.add_dummy_triplets = wrapped
            groups = []
            for gi, group in enumerate(GROUPS):
                random.seed(seed * 100 + gi)
                np.random.seed(seed * 100 + gi)
                del rec.log[:], at_dummies[:]
                samples = [ds[i] for i in group]
                _, objs, boxes, triplets, conv_counts, ttype, masks, ids = coco_collate_fn(ds.vocab, samples)
                assert masks is None and ids.tolist() == [SAMPLES[i][0] for i in group] and boxes.dtype == torch.float32
                B, Og = len(group), objs.shape[1] - 1
                other = np.full((B, Og), -1, np.int32)
                flip = np.zeros((B, Og), np.uint8)
                rows = np.zeros((B, Og, 3), np.int64)
                rows[:, :, 1] = ds.vocab["pred_name_to_idx"]["__padding__"]
                log = list(rec.log)
                for b, i in enumerate(group):
                    n = len(SAMPLES[i][2])
                    drawn = n if (rels and n >= 2) else 0
                    assert len(at_dummies[b]) == drawn
                    for cur in range(drawn):
                        (k0, j), (k1, u) = log.pop(0), log.pop(0)
                        assert k0 == "choice" and k1 == "random"
                        other[b, cur], flip[b, cur] = j, 0 if u > 0.5 else 1
                        rows[b, cur] = at_dummies[b][cur]
                        s, o = (j, cur) if flip[b, cur] else (cur, j)
                        d = boxes[b, s, :2] + 0.5 * boxes[b, s, 2:] - (boxes[b, o, :2] + 0.5 * boxes[b, o, 2:])
                        dx, dy = float(d[0]), float(d[1])
                        if abs(dx) == abs(dy) or dx == 0 or dy == 0:
                            seen.add((int(np.sign(dx)), int(np.sign(dy))))
                        seen.add(ds.vocab["pred_idx_to_name"][rows[b, cur, 1]])
                assert not log
                tag = "s%d_g%d_" % (si, gi)
                arrays.update({tag + "objs": mg.npy(objs[:, :, 0]).astype(np.int16), tag + "boxes": mg.npy(boxes),
                               tag + "other": other, tag + "flip": flip, tag + "rows": rows.astype(np.int16),
                               tag + "triplets": mg.npy(triplets).astype(np.int16), tag + "tt": mg.npy(ttype).astype(np.int8),
                               tag + "conv": mg.npy(conv_counts).astype(np.int16)})
                groups.append({"samples": list(group), "seed": seed * 100 + gi, "objects": list(objs.shape),
                               "triplets": list(triplets.shape), "converse_draws": int(conv_counts.sum())})
            settings.append({"use_converse": conv, "learned_transitivity": trans, "include_relationships": rels,
                             "learned_converse": lconv, "groups": groups})
            vocab = ds.vocab
    ties = {(1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0), (0, -1), (-1, 0)}
    assert ties <= seen, "tie directions not met by these seeds: %s" % sorted(ties - seen)
    assert {"__surrounding__", "__inside__", "__left of__", "__right of__", "__above__", "__below__"} <= seen, seen
    mg.save("coco_pairs", {"ref": "sg2im/data/coco.py:287-430 (__getitem__), :452-545 (coco_collate_fn); "
                                  "sg2im/data/base_dataset.py:89-162",
                           "substitution": "seg_to_mask and cv2.resize return zeros: every mask is empty, so the reference "
                                           "takes its fallback centre x0 + 0.5 * w, y0 + 0.5 * h (coco.py:356-358)",
                           "python": platform.python_version(), "numpy": np.__version__,
                           "instance_categories": [list(c) for c in INSTANCE_CATEGORIES],
                           "stuff_categories": [list(c) for c in STUFF_CATEGORIES],
                           "object_name_to_idx": vocab["object_name_to_idx"], "pred_name_to_idx": vocab["pred_name_to_idx"],
                           "pred_idx_to_name": vocab["pred_idx_to_name"], "sizes": "(HH, WW) of the decoded pictures",
                           "boxes_px": "x, y, w, h in pixels, -1 in padding rows; cats 0 there", "settings": settings,
                           "dtypes": "objs / rows / triplets / conv int16, tt int8 (int64, conv float32 in the collate); "
                                     "rows = the triplets as they stand when add_dummy_triplets is called, [0, __padding__, "
                                     "0] beyond; other int32 (-1 beyond), flip uint8: what random.choice / random.random "
                                     "returned, flip = not (u > 0.5)"},
            **arrays)
    for s in settings:
        print(s)


if __name__ == "__main__":
    torch.set_num_threads(4)
    fx_coco_pairs()
