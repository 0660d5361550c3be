#!/usr/bin/env python3
"""Generate tests/golden/clevr_unpacked.npz by running the REAL reference's unpacked CLEVR loader on the CPU: the
module-level functions of sg2im/data/clevr_dialog.py that its __getitem__ calls — extract_triplets (:289-307, with
scripts/graphs_utils.py's reduce_transitive_edges), extract_objs (:227-233), extract_bounding_boxes (:21-77) and the
`[0, 0, 1, 1]` row of :176-179 — then clevr_collate_fn_fix (:387-463), on the hand-made scenes of
tests/clevr_graph_cases.py, for use_transitivity 0 and 1.  Every case is collated alone, and the cases of `MIXED` as one
batch, so that objects, boxes and triplets all get padded.

The vocabulary is the one the reference's constructor builds (:94-122): the dataset is constructed once, on a temporary
folder that holds the scenes file and the dialog file.  reduce_transitive_edges draws from numpy's GLOBAL stream; it is seeded
before every collated batch (the result does not depend on it for 0 and 1, the metadata records the seed all the same).
Needs the reference checkout (build container only, through make_golden's import shim); the output is plain tensors + JSON
metadata.
Usage:  python tests/golden/make_golden_clevr_unpacked.py
"""
import json
import os
import platform
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the reference import shim, npy)

import clevr_graph_cases as gc  # noqa: E402  (ours: the scenes)

SEED = 31


def sample(ref, scene, vocab, keep):
    """What CLEVRDialogDataset.__getitem__ returns for a scene (:172-181), the picture apart."""
    triplets = ref.extract_triplets(scene, vocab, use_transitivity=keep)
    objs = ref.extract_objs(scene, vocab)
    x, y, w, h = ref.extract_bounding_boxes(scene)
    boxes = list(zip(x, y, w, h))
    boxes.append([0., 0., 1., 1.])
    return torch.zeros(3, 4, 4), objs, torch.FloatTensor(boxes), triplets, scene


def main():
    import sg2im.data.clevr_dialog as ref
    scenes = {name: gc.scene_dict(name) for name in gc.NAMES}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "scenes"))
        with open(os.path.join(tmp, "scenes", "CLEVR_train_scenes.json"), "w") as f:
            json.dump({"scenes": list(scenes.values())}, f)
        with open(os.path.join(tmp, "dialog.json"), "w") as f:
            json.dump([{"split": s["split"], "image_filename": s["image_filename"]} for s in scenes.values()], f)
        vocab = ref.CLEVRDialogDataset("dialog.json", tmp, "train").vocab
    arrays, counts = {}, {}
    for keep in (0, 1):
        for tag, names in [(name, (name,)) for name in gc.NAMES] + [("mixed", gc.MIXED)]:
            np.random.seed(SEED)
            items = [sample(ref, scenes[name], vocab, keep) for name in names]
            _, objs, boxes, triplets, ids, _ = ref.clevr_collate_fn_fix(vocab, items)
            assert objs.dtype == torch.int64 and boxes.dtype == torch.float32 and triplets.dtype == torch.int64
            assert ids.tolist() == [scenes[name]["image_index"] for name in names]
            arrays["%s_k%d_triplets" % (tag, keep)] = mg.npy(triplets).astype(np.int16)
            counts["%s_k%d" % (tag, keep)] = [int(it[3].shape[0]) for it in items]
            if keep == 0:
                arrays[tag + "_objs"] = mg.npy(objs).astype(np.int8)
                arrays[tag + "_boxes"] = mg.npy(boxes)
    meta = {"ref": "sg2im/data/clevr_dialog.py:21-77, :94-122, :172-181, :227-233, :289-307, :387-463; "
                   "scripts/graphs_utils.py:15-44, :47-61, :74-82",
            "vocab": {"pred_name_to_idx": vocab["pred_name_to_idx"],
                      "pred_idx_to_name": [vocab["pred_idx_to_name"][i] for i in range(len(vocab["pred_idx_to_name"]))],
                      "attributes": vocab["attributes"], "object_name_to_idx": vocab["object_name_to_idx"],
                      "use_object_embedding": vocab["use_object_embedding"]},
            "cases": list(gc.NAMES), "mixed": list(gc.MIXED), "counts": counts, "seed": SEED,
            "python": platform.python_version(), "numpy": np.__version__,
            "dtypes": "triplets int16, objs int8 (int64 in the collate), boxes float32; <case>_k<use_transitivity>_triplets "
                      "(1,T,3), mixed_* (4,..); counts = triplets per sample before the collate's padding; numpy's global "
                      "stream is seeded with `seed` before every collated batch"}
    path = os.path.join(HERE, "clevr_unpacked.npz")
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print("%s %.1f KB %d arrays" % (path, os.path.getsize(path) / 1024, len(arrays)))
    print(counts)


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
