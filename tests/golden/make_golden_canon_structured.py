#!/usr/bin/env python3
"""Generate tests/golden/canon_structured.npz by running the REAL reference on CPU over the structured scene families of
tests/canon_cases.py at small sizes (at most 12 rows per sample).

Per case one sample, through BaseDataset.add_location_triplets -> add_dummy_triplets -> add_learnt_triplets
(sg2im/data/base_dataset.py:35-151) in the order of packed_clevr_dialog.py:205-209, for both learned_transitivity settings,
without and with learned_converse (numpy's GLOBAL stream, seeded per run, as make_golden.fx_canon_converse does).  A case
the reference itself cannot build — no location triplet at all (it indexes an empty array), no `__image__` row or two of
them with include_dummies (it squeezes the index of the row to an int) — is recorded as such in the metadata, with the
exception's type, and carries no arrays.  Needs the reference checkout (build container only); the output is plain tensors
+ JSON metadata.  Usage:  python tests/golden/make_golden_canon_structured.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the reference import shim, save / npy)

import canon_cases as cc  # noqa: E402  (ours: inputs only)
from canonicalsg2im_amd.synth import make_vocab  # noqa: E402

# (family, rows with the __image__ rows, where they sit, include_dummies, family keywords)
CASES = (
    ("random", 12, "last", 1, {}), ("chain", 6, "last", 1, {}), ("chain", 12, "last", 1, {}), ("reverse_chain", 7, "last", 1, {}),
    ("shuffled_chain", 12, "last", 1, {}), ("nested", 9, "last", 1, {}), ("nested", 10, "last", 1, {"odd_seed": True}),
    ("identical", 5, "last", 1, {}), ("grid", 10, "last", 1, {}), ("grid", 12, "last", 1, {}),
    ("two_clusters", 11, "last", 1, {"split": 5}), ("two_clusters", 11, "last", 1, {"split": 5, "bridge": True}),
    ("single", 2, "last", 1, {}), ("only_image", 1, "last", 1, {}),
    ("random", 9, "first", 1, {}), ("random", 9, "middle", 1, {}), ("chain", 8, "first", 1, {}), ("chain", 8, "middle", 1, {}),
    ("random", 9, "absent", 1, {}), ("random", 9, "twice", 1, {}), ("random", 9, "absent", 0, {}), ("random", 9, "twice", 0, {}),
    ("shuffled_chain", 10, "twice", 0, {}), ("nested", 8, "middle", 0, {}),
)


def fx_canon_structured():
    from sg2im.data.base_dataset import BaseDataset
    vocab = make_vocab("clevr")
    P = len(vocab["pred_name_to_idx"])
    arrays, cases = {}, []
    w = torch.from_numpy(np.random.default_rng(900).normal(size=(P, P)).astype(np.float32))
    up = torch.triu(w, diagonal=0)
    weights = (up + up.t()).detach().cpu().numpy()                                      # model.py:10-13, train.py:276
    arrays["weights"] = weights
    for ci, (family, rows, image, dummies, kw) in enumerate(CASES):
        kw = dict(kw)
        seed = 40 + 2 * ci + (1 if kw.pop("odd_seed", False) else 0)
        objs, boxes, centers = cc.sample(family, rows, seed, image, **kw)
        tag = "c%d_" % ci
        case = {"family": family, "rows": rows, "image": image, "include_dummies": dummies, "kw": kw, "seed": seed, "runs": []}
        arrays[tag + "in"] = np.concatenate([objs[:, None].astype(np.float32), boxes, centers], axis=1)
        packed, convs = [], []
        for trans in (0, 1):
            for conv in (0, 1):
                ds = BaseDataset()
                ds.vocab, ds.include_dummies = vocab, bool(dummies)
                ds.learned_transitivity, ds.learned_converse, ds.learned_symmetry = bool(trans), bool(conv), False
                ds.converse_candidates_weights = weights
                np_seed = 7000 + 10 * ci + 2 * trans + conv
                np.random.seed(np_seed)
                run = {"learned_transitivity": trans, "learned_converse": conv, "seed": np_seed}
                try:
                    triplets = []
                    o = torch.from_numpy(objs)
                    ds.add_location_triplets(torch.from_numpy(boxes), torch.from_numpy(centers), o, triplets)
                    ds.add_dummy_triplets(o, triplets)
                    triplets, conv_counts, ttype = ds.add_learnt_triplets(triplets, rows)
                    t = np.asarray(triplets, np.int64).reshape(-1, 3)
                    packed.append(np.concatenate([t, np.asarray(ttype, np.int64).reshape(-1, 1)], axis=1).astype(np.int8))
                    run["count"] = len(t)
                    if conv:
                        convs.append(np.asarray(conv_counts, np.float32))
                    run["draws"] = int(np.asarray(conv_counts).sum())
                    run["refused"] = None
                except Exception as e:                   # the reference cannot build this graph: recorded, not compared
                    run["refused"] = type(e).__name__
                case["runs"].append(run)
        if packed:                                       # the runs' rows [s, p, o, type] one after the other; conv per converse run
            arrays[tag + "rows"] = np.concatenate(packed, axis=0)
            arrays[tag + "conv"] = np.stack(convs).astype(np.int16)
        cases.append(case)
        print("%-16s rows %2d image %-6s dummies %d: %s" % (family, rows, image, dummies,
                                                              [r["refused"] or "ok" for r in case["runs"]]))
    mg.save("canon_structured", {"ref": "sg2im/data/base_dataset.py:35-151; scripts/graphs_utils.py:15-100,126-152; "
                                        "sg2im/data/packed_clevr_dialog.py:205-209",
                                 "vocab": "clevr", "cases": cases,
                                 "layout": "c<i>_in (rows,7) float32 = objs | boxes | centers; c<i>_rows int8 = [s, p, o, triplet_type] of the "
                                           "case's runs one after the other (run['count'] each, unpadded); c<i>_conv int16 = "
                                           "conv_counts (P,P+1) of its learned_converse runs in order; weights (P,P) shared"},
            **arrays)


if __name__ == "__main__":
    torch.set_num_threads(4)
    fx_canon_structured()
