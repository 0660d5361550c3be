#!/usr/bin/env python
"""Generate tests/golden/clevr_syn.npz by running the REAL reference's synthetic CLEVR scenes (sg2im/data/packed_clevr_dialog.py).

Needs a checkout of the reference, named on the command line.  The module's imports need cv2 and matplotlib, so its two
dataset classes and its collate are taken from the module's source by their AST and executed on their own, over the
reference's own BaseDataset (by its AST too: the package's __init__ needs torchvision) and scripts/graphs_utils.py (imported
from the checkout: it needs torch, numpy and scipy alone).
Nothing of the reference travels: the output is recorded data + JSON metadata.

(a) scenes: `create_packed_sgs` (:577-628; the text of :464-515 is the same, but there `add_location_triplets` is handed
    `objs=None`, which BaseDataset's reads) after `random.seed(seed); np.random.seed(seed)`, for seeds 0 and 1 and
    (min_objects, max_objects) = (1,1), (3,3), (15,30): per object the four attribute ids and the fp64 box.
(b) batches: PackedGenCLEVRDataset.__getitem__ (:410-452) of those scenes + packed_clevr_collate_fn (:253-334), with
    learned_transitivity 0 and 1: objs, boxes, centres (the fp32 tensor __getitem__ hands to add_location_triplets),
    triplets, triplet_type.
(c) verdicts: PackedSynCLEVRDataset.add_location_triplets (:672-716: the pair rule alone, no reduction) on PERTURBED fp32
    copies of some scenes' boxes inside [0,1] — coarse-grid values, so exact ties in x0 and in the centres occur, and
    nested pairs both ways: every (s, p, o) the reference says holds.

    python tests/golden/make_golden_clevr_syn.py REFERENCE_CHECKOUT
"""
import ast
import copy
import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join("sg2im", "data", "packed_clevr_dialog.py")       # under the reference checkout
BASE = os.path.join("sg2im", "data", "base_dataset.py")
GROUPS = [(1, 1, 3), (3, 3, 3), (15, 30, 4)]                           # (min_objects, max_objects, max_samples)
SEEDS = [0, 1]
ATTRS = ["shape", "color", "material", "size"]                          # the vocabulary's attribute order = objs columns


def reference_classes(checkout):
    sys.path.insert(0, checkout)
    import scripts.graphs_utils as gu
    # sg2im.data's __init__ imports torchvision: BaseDataset and the edge-type constants by their AST as well
    tree = ast.parse(open(os.path.join(checkout, BASE)).read(), BASE)
    body = [n for n in tree.body if isinstance(n, ast.Assign) or (isinstance(n, ast.ClassDef) and n.name == "BaseDataset")]
    base = {"torch": torch, "np": np, "Dataset": torch.utils.data.Dataset}
    for name in ("get_edge_converse_triplets", "get_current_and_transitive_triplets", "triplets_to_minimal"):
        base[name] = getattr(gu, name)
    exec(compile(ast.Module(body=body, type_ignores=[]), BASE, "exec"), base)
    bd = types.SimpleNamespace(**base)
    tree = ast.parse(open(os.path.join(checkout, SOURCE)).read(), SOURCE)
    want = ("PackedGenCLEVRDataset", "PackedSynCLEVRDataset", "packed_clevr_collate_fn")
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in want]
    assert len(body) == 3
    none = lambda *a, **k: None
    scope = {"random": random, "np": np, "torch": torch, "os": os, "BaseDataset": bd.BaseDataset,
             "T": types.SimpleNamespace(ToTensor=none, Compose=none), "Resize": none, "encode_image": none,
             "ORIGINAL_EDGE": bd.ORIGINAL_EDGE, "TRANSITIVE_EDGE": bd.TRANSITIVE_EDGE,
             "SYMMETRIC_EDGE": bd.SYMMETRIC_EDGE, "ANTI_SYMMETRIC_EDGE": bd.ANTI_SYMMETRIC_EDGE}
    for name in ("get_minimal_and_transitive_triplets", "get_symmetric_triplets", "get_current_and_transitive_triplets",
                 "get_edge_converse_triplets"):
        scope[name] = getattr(gu, name)
    exec(compile(ast.Module(body=body, type_ignores=[]), SOURCE, "exec"), scope)
    return scope


def perturbed(n, rng):
    """fp32 boxes inside [0,1] on a grid of 1/16: ties in x0 and in the centres, and nested pairs both ways."""
    x0 = rng.integers(0, 9, size=(n, 2)) / 16.0
    wh = rng.integers(1, 8, size=(n, 2)) / 16.0
    return np.concatenate([x0, wh], 1).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = reference_classes(sys.argv[1])
    Gen, Syn, collate = ref["PackedGenCLEVRDataset"], ref["PackedSynCLEVRDataset"], ref["packed_clevr_collate_fn"]
    arrays, meta = {}, {"source": "sg2im/data/packed_clevr_dialog.py:253-334,410-452,577-628,672-716 over "
                                  "sg2im/data/base_dataset.py:35-139, run by make_golden_clevr_syn.py",
                        "seeds": SEEDS, "groups": GROUPS, "attributes": ATTRS, "runs": [], "verdicts": []}
    rng = np.random.default_rng(11)
    for seed in SEEDS:
        for lo, hi, count in GROUPS:
            random.seed(seed)
            np.random.seed(seed)
            syn = Syn("", "val", min_objects=lo, max_objects=hi, max_samples=count)
            scenes = syn.data
            key = "s%d_%d_%d" % (seed, lo, hi)
            meta["runs"].append({"key": key, "seed": seed, "min_objects": lo, "max_objects": hi, "max_samples": count})
            table = syn.vocab["attributes"]
            counts = np.asarray([len(s["objects"]) for s in scenes], np.int64)
            ids = np.zeros((count, counts.max(), 4), np.int64)
            boxes = np.zeros((count, counts.max(), 4), np.float64)
            for b, s in enumerate(scenes):
                assert s["image_index"] == str(b)
                ids[b, :counts[b]] = [[table[a][o[a]] for a in ATTRS] for o in s["objects"]]
                boxes[b, :counts[b]] = s["boxes"]
            arrays[key + "_counts"], arrays[key + "_ids"], arrays[key + "_boxes64"] = counts, ids.astype(np.int16), boxes
            for lt in (0, 1):
                gen = Gen("", "val", min_objects=lo, max_objects=hi, max_samples=count, learned_transitivity=bool(lt),
                          include_dummies=True)
                gen.data = copy.deepcopy(scenes)                     # __getitem__ appends the __image__ box to its scene
                centres = []
                keep = gen.add_location_triplets
                gen.add_location_triplets = lambda bx, ce, ob, tr, keep=keep: (centres.append(ce.clone()), keep(bx, ce, ob, tr))[1]
                if hi < 2:            # one object: no location triplet, and the reference indexes the empty array (:85)
                    try:
                        gen[0]
                    except IndexError:
                        meta["runs"][-1]["getitem"] = "IndexError"
                        continue
                items = [gen[i] for i in range(count)]
                # the collate indexes the picture and makes a LongTensor of the ids: a stand-in picture, the id as a number
                _, objs, bx, trip, _, ttype, masks, image_ids = collate(
                    gen.vocab, [(torch.zeros(1),) + it[1:7] + (int(it[7]),) for it in items])
                assert masks is None and image_ids.tolist() == list(range(count))
                assert all(it[0] is None and it[7] == str(i) for i, it in enumerate(items))
                ce = np.zeros((count, bx.shape[1], 2), np.float32)
                for b, c in enumerate(centres):
                    ce[b, :c.shape[0]] = c.numpy()
                pre = "%s_lt%d_" % (key, lt)
                arrays[pre + "objs"], arrays[pre + "boxes"] = objs.numpy().astype(np.int16), bx.numpy()
                arrays[pre + "centers"], arrays[pre + "triplets"] = ce, trip.numpy().astype(np.int16)
                arrays[pre + "triplet_type"] = ttype.numpy().astype(np.int8)
            # (c) the pair rule on perturbed boxes
            for b in (0, count - 1):
                n = int(counts[b])
                if n < 2:
                    continue
                p = perturbed(n, rng)
                bt = torch.from_numpy(p)
                ce = bt[:, :2] + 0.5 * bt[:, 2:]
                out = []
                syn.add_location_triplets(bt, ce, None, out)
                vk = "%s_v%d_" % (key, b)
                meta["verdicts"].append(vk)
                arrays[vk + "boxes"], arrays[vk + "centers"] = p, ce.numpy()
                arrays[vk + "holds"] = np.asarray(out, np.int16).reshape(-1, 3)
    meta["pred_name_to_idx"] = syn.vocab["pred_name_to_idx"]
    names = {syn.vocab["pred_idx_to_name"][int(p)] for k in meta["verdicts"] for p in arrays[k + "holds"][:, 1]}
    assert names == set(syn.augmented_relations), names           # every location predicate, the nested ones included
    out = os.path.join(HERE, "clevr_syn.npz")
    np.savez_compressed(out, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(out, os.path.getsize(out), "bytes", len(arrays), "arrays", file=sys.stderr)
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
