#!/usr/bin/env python3
"""Generate tests/golden/authored_graphs.npz by running the REAL reference on CPU: the twelve authored scene graphs of its
scripts/run_model.py (auto_create_graphs(3..6), each as sparse, dense and hyper graph, :56-103) encoded by its
extract_objs / extract_triplets (sg2im/data/clevr_dialog.py:227-233, 289-307) over a CLEVR vocabulary.

The vocabulary is CLEVRDialogDataset's (clevr_dialog.py:94-106: four attributes, the predicates __in_image__, right, behind,
front, left, __padding__) with the six location relations appended by OUR register_augmented_relations, as the packed
loaders do (base_dataset.py:153-162): the canonical-graph kernels need them in the role table.  It is written into the
fixture as names and ids.  Needs the reference checkout (build container only); the output holds the graphs as JSON, the
vocabulary as JSON and the encoded arrays: names and numbers, no program text.
Usage:  python tests/golden/make_golden_authored.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (the reference import shim, save / npy)

from canonicalsg2im_amd.sg2im.data.base_dataset import register_augmented_relations  # noqa: E402  (ours)


def clevr_vocab():
    vocab = {"attributes": {
        "shape": {"__image__": 0, "cube": 1, "sphere": 2, "cylinder": 3},
        "color": {"__image__": 0, "gray": 1, "red": 2, "blue": 3, "green": 4, "brown": 5, "purple": 6, "cyan": 7, "yellow": 8},
        "material": {"__image__": 0, "rubber": 1, "metal": 2},
        "size": {"__image__": 0, "small": 1, "large": 2}}}
    names = ["__in_image__", "right", "behind", "front", "left", "__padding__"]
    vocab["pred_name_to_idx"] = {n: i for i, n in enumerate(names)}
    vocab["pred_idx_to_name"] = list(names)
    return register_augmented_relations(vocab)


def fx_authored():
    import matplotlib
    matplotlib.use("Agg")
    from scripts.run_model import scene_graphs                                  # reference: the twelve graphs
    from sg2im.data.clevr_dialog import extract_objs, extract_triplets          # reference
    assert len(scene_graphs) == 12
    vocab = clevr_vocab()
    attrs = list(vocab["attributes"].keys())
    arrays, sizes = {}, []
    for g, sg in enumerate(scene_graphs):
        np.random.seed(g)               # reduce_transitive_edges draws a matrix that decides nothing at p_keep = 0
        objs = extract_objs(sg, vocab)
        trip = extract_triplets(sg, vocab)
        arrays["g%d_objs" % g] = np.stack([mg.npy(objs[a]) for a in attrs], axis=1).astype(np.int64)     # (n + 1, A)
        arrays["g%d_triplets" % g] = mg.npy(trip).astype(np.int64)
        sizes.append(len(sg["objects"]))
    mg.save("authored_graphs", {"ref": "scripts/run_model.py:44-103; sg2im/data/clevr_dialog.py:227-233,289-307; "
                                       "scripts/graphs_utils.py:15-82",
                                "graphs": scene_graphs, "sizes": sizes, "kinds": ["sparse", "dense", "hyper"] * 4,
                                "attributes": vocab["attributes"], "pred_idx_to_name": vocab["pred_idx_to_name"]},
            **arrays)


if __name__ == "__main__":
    fx_authored()
