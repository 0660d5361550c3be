#!/usr/bin/env python3
"""Generate tests/golden/canon_annotated.npz by running the REAL reference on CPU: the canonical graphs of the packed
Visual Genome loader, annotated relationships included.

Per sample, in the order of sg2im/data/packed_vg.py:127-142: the annotated rows, BaseDataset.add_location_triplets,
add_dummy_triplets, add_learnt_triplets (sg2im/data/base_dataset.py:35-151); then vg_collate_fn (packed_vg.py:154-229).
With learned_converse the draws come from numpy's GLOBAL stream, seeded per case (as make_golden.fx_canon_converse does).
Needs the reference checkout (build container only); the output is plain tensors + JSON metadata.
Usage:  python tests/golden/make_golden_annotated.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (the reference import shim, save / npy)

from canonicalsg2im_amd.synth import annotated_relations, make_vocab  # noqa: E402  (ours: inputs only)

# (real objects per sample, learned_transitivity, learned_converse, seed of numpy's global stream, permuted ids)
CASES = (
    ((2, 3, 7, 20, 55, 100), 0, 0, 31, False),
    ((2, 5, 12, 24), 1, 0, 32, False),
    ((3, 9, 40, 100), 0, 1, 33, False),
    ((2, 6, 17, 30), 1, 1, 34, False),
    ((4, 11, 25), 1, 1, 35, True),
    ((3, 60, 21), 0, 1, 36, True),
    ((250,), 0, 1, 37, False),
)


def _vocab(permuted, rng):
    vocab = make_vocab("vg")
    if permuted:                       # location and meta predicates anywhere among the ids
        names = list(vocab["pred_idx_to_name"])
        names = [names[i] for i in rng.permutation(len(names))]
        vocab["pred_idx_to_name"] = names
        vocab["pred_name_to_idx"] = {nm: i for i, nm in enumerate(names)}
    return vocab


def _annotated(rng, n, vocab, empty):
    """annotated_relations plus rows whose predicate is a location relation (never reduced by the reference)."""
    if empty:
        return []
    rows = annotated_relations(rng, n, vocab)
    p2i = vocab["pred_name_to_idx"]
    for name in ("__left of__", "__inside__"):
        s, o = (int(v) for v in rng.choice(n, size=2, replace=False))
        rows.append([s, p2i[name], o])
    return rows


def fx_canon_annotated():
    from sg2im.data.base_dataset import BaseDataset
    from sg2im.data.packed_vg import vg_collate_fn
    rng = np.random.default_rng(4242)
    arrays, cases = {}, []
    for ci, (sizes, trans, conv, seed, permuted) in enumerate(CASES):
        vocab = _vocab(permuted, rng)
        P = len(vocab["pred_name_to_idx"])
        image_id = vocab["object_name_to_idx"]["__image__"]
        ds = BaseDataset()
        ds.vocab, ds.include_dummies = vocab, True
        ds.learned_transitivity, ds.learned_converse, ds.learned_symmetry = bool(trans), bool(conv), False
        w = torch.from_numpy(rng.normal(size=(P, P)).astype(np.float32))
        up = torch.triu(w, diagonal=0)
        ds.converse_candidates_weights = (up + up.t()).detach().cpu().numpy()          # model.py:10-13, train.py:276
        np.random.seed(seed)
        batch, rels, centers = [], [], []
        for k, n in enumerate(sizes):
            wh = rng.uniform(0.05, 0.6, size=(n, 2))
            xy = rng.uniform(0.0, 1.0, size=(n, 2)) * (1.0 - wh)
            if n >= 6:                                       # exact ties of centres / edges exercise the strict compares
                xy[1] = xy[0]; wh[1] = wh[0]
                xy[3, 0] = xy[2, 0]
            O = n + 1                                        # the __image__ object last (packed_vg.py:112-123)
            objs = torch.LongTensor(list(rng.integers(1, len(vocab["object_idx_to_name"]), size=n)) + [image_id])
            boxes = torch.FloatTensor([[-1, -1, -1, -1]]).repeat(O, 1)
            boxes[:n] = torch.FloatTensor(np.concatenate([xy, wh], axis=1))
            obj_centers = torch.stack([boxes[:, 0] + (boxes[:, 2] / 2), boxes[:, 1] + (boxes[:, 3] / 2)], dim=1)
            triplets = _annotated(rng, n, vocab, empty=(k == 1))         # the second sample has no relationships
            rels.append(np.asarray(triplets, np.int64).reshape(-1, 3))
            ds.add_location_triplets(boxes, obj_centers, objs, triplets)
            ds.add_dummy_triplets(objs, triplets)
            triplets, conv_counts, ttype = ds.add_learnt_triplets(triplets, objs.size(0))
            batch.append((torch.zeros(1, 3, 4, 4), {"objects": objs}, boxes, torch.LongTensor(triplets),
                          torch.FloatTensor(conv_counts), torch.LongTensor(ttype), None, k))
            centers.append(obj_centers)
        draws = int(sum(float(b[4].sum()) for b in batch))
        _, all_objs, all_boxes, all_triplets, all_conv, all_tt, _, _ = vg_collate_fn(vocab, batch)
        B, O = all_boxes.shape[:2]
        cen = torch.zeros(B, O, 2)
        for b, n in enumerate(sizes):
            cen[b, :n + 1] = centers[b]
        R = max(len(r) for r in rels)
        rel = np.zeros((B, R, 3), np.int64)
        rel[:, :, 1] = vocab["pred_name_to_idx"]["__padding__"]
        for b, r in enumerate(rels):
            rel[b, :len(r)] = r
        tag = "c%d_" % ci
        arrays.update({tag + "objs": mg.npy(all_objs[:, :, 0]).astype(np.int16), tag + "boxes": mg.npy(all_boxes),
                       tag + "centers": mg.npy(cen), tag + "n": np.asarray([n + 1 for n in sizes], np.int64),
                       tag + "rel": rel.astype(np.int16), tag + "triplets": mg.npy(all_triplets).astype(np.int16),
                       tag + "tt": mg.npy(all_tt).astype(np.int8),
                       tag + "counts": np.asarray([len(b[3]) for b in batch], np.int64)})
        if conv:
            arrays[tag + "weights"] = ds.converse_candidates_weights.copy()
            nz = mg.npy(all_conv).reshape(B * P, P + 1)              # conv_counts: mostly zero rows, stored sparse
            rows = np.nonzero(nz.any(axis=1))[0]
            arrays.update({tag + "conv_rows": rows.astype(np.int32), tag + "conv_vals": nz[rows].astype(np.float32)})
        cases.append({"sizes": list(sizes), "learned_transitivity": trans, "learned_converse": conv, "seed": seed,
                      "draws": draws, "pred_idx_to_name": vocab["pred_idx_to_name"]})
    mg.save("canon_annotated", {"ref": "sg2im/data/packed_vg.py:127-142,154-229; sg2im/data/base_dataset.py:35-151; "
                                       "scripts/graphs_utils.py:15-100,126-152",
                                "vocab": "vg", "cases": cases,
                                "dtypes": "objs / rel / triplets int16, tt int8 (int64 in the collate); conv_counts "
                                          "(B,P,P+1) float32 as the rows of its (B*P, P+1) view that hold a draw"},
            **arrays)


if __name__ == "__main__":
    torch.set_num_threads(4)
    fx_canon_annotated()
