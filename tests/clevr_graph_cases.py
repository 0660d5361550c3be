"""The unpacked CLEVR dataset's graph: the case table, a bit-row restatement of the rule the device code follows, and a small
folder in the reference's layout (tests/test_clevr_graph_cases.py pins them to the reference's recorded output on the CPU,
tests/test_gpu_clevr_unpacked.py holds csrc/clevr_graph.hip and the dataset to them).

Reference: extract_triplets (sg2im/data/clevr_dialog.py:289-307) lists, per key of the scene's `relationships` and then per
o1 ascending, a row [o2, pred, o1] for every o2 of `relationships[key][o1]`, and hands each key's rows to
reduce_transitive_edges (scripts/graphs_utils.py:74-82).  The rule, for a key's rows:
  fewer than 3 rows: as listed;
  otherwise M = the rows as a matrix, C = path(M) (Warshall, pivot i: every row j != i with bit i takes row i),
  H = hsu(C) in the reference's in-place order — with old = row j before step j and self = bit j of old: rows i < j with
  bit j clear old; row j becomes 0 if self; rows i > j with bit j clear old only if not self — and the rows of H
  (use_transitivity 0) or H | M (use_transitivity 1), row-major.
Then [i, __in_image__, n] per object.  Integers throughout: equality, no tolerance."""
import json
import os

import numpy as np

PREDS = {"__in_image__": 0, "right": 1, "behind": 2, "front": 3, "left": 4, "__padding__": 5}      # clevr_dialog.py:96-97
KEYS = ("right", "behind", "front", "left")              # the key order of CLEVR's scene files
SHAPES, MATERIALS, SIZES = ("cube", "sphere", "cylinder"), ("rubber", "metal"), ("small", "large")
COLORS = ("gray", "red", "blue", "green", "brown", "purple", "cyan", "yellow")
MIXED = ("one", "three_order", "ten_orders", "n63")      # the batch whose objects, boxes and triplets all get padded
FOLDER_MODES = ("RGBA", "RGB", "RGBA", "RGB")
FOLDER_SIZES = ((32, 48), (37, 53), (64, 64), (40, 60))  # (h, w) of the folder's pictures, MIXED's scenes in order


def order_rel(perm):
    """relationships[key] of a strict total order: perm[k] is the object of rank k, and relationships[key][o1] lists the
    objects of higher rank, by rank — so not by ascending index."""
    rank = {o: k for k, o in enumerate(perm)}
    return [[o2 for o2 in perm if rank[o2] > rank[o1]] for o1 in range(len(perm))]


def edges_rel(n, edges):
    """relationships[key] with the row [s, pred, o] for every (s, o) of `edges`: s joins relationships[key][o], in order."""
    rel = [[] for _ in range(n)]
    for s, o in edges:
        rel[o].append(s)
    return rel


def _perm(n, seed):
    return [int(i) for i in np.random.default_rng(seed).permutation(n)]


def _none(n):
    return [[] for _ in range(n)]


def _scenes():
    """name -> (objects, relationships as an ordered dict of key -> per-object lists)."""
    s = {}
    s["one"] = (1, {k: _none(1) for k in KEYS})                                        # no relation row: the dummy alone
    s["two"] = (2, {"right": [[1], []], "behind": [[], [0]], "front": [[1], []], "left": [[], [0]]})   # one row each: listed
    s["three_order"] = (3, {k: order_rel(_perm(3, 40 + i)) for i, k in enumerate(KEYS)})  # 3 rows -> a chain of 2
    s["ten_orders"] = (10, {k: order_rel(_perm(10, 50 + i)) for i, k in enumerate(KEYS)})  # CLEVR's largest scene
    s["dup2"] = (3, {"right": [[1, 1], [], []], "behind": _none(3), "front": _none(3), "left": _none(3)})  # both are kept
    s["dup3"] = (3, {"right": [[1, 1, 2], [], []], "behind": _none(3), "front": _none(3), "left": _none(3)})  # merged
    # two rows, listed [2, p, 0] then [0, p, 1]: row-major order would turn them round
    s["listed_order"] = (3, {"right": [[2], [0], []], "behind": _none(3), "front": [[], [2], [1]], "left": _none(3)})
    s["cycle_chain"] = (5, {"right": edges_rel(5, [(0, 1), (1, 0), (2, 3), (3, 4)]), "behind": _none(5),
                            "front": edges_rel(5, [(4, 3), (3, 4), (1, 3), (0, 1)]), "left": _none(5)})
    s["self_relation"] = (4, {"right": edges_rel(4, [(0, 1), (1, 1), (1, 2)]), "behind": edges_rel(4, [(2, 2), (0, 2), (3, 0)]),
                              "front": edges_rel(4, [(0, 0), (1, 1), (3, 3)]), "left": edges_rel(4, [(3, 3), (3, 1), (1, 0), (0, 2)])})
    s["open_dag"] = (4, {"right": edges_rel(4, [(0, 1), (1, 2), (0, 2), (2, 3)]), "behind": _none(4), "front": _none(4),
                         "left": _none(4)})                                              # a->b, b->c, a->c, c->d: keep differs
    s["key_order"] = (3, {k: order_rel(_perm(3, 60 + i)) for i, k in enumerate(("left", "front", "right", "behind"))})
    s["n63"] = (63, {k: order_rel(_perm(63, 70 + i)) for i, k in enumerate(KEYS)})      # lane 62, the __image__ row 63
    return s


SCENES = _scenes()
NAMES = tuple(SCENES)


def scene_dict(name, split="train"):
    """The scene file's record of a case: seeded attributes and geometry in CLEVR's ranges, the case's relationships."""
    n, rel = SCENES[name]
    i = NAMES.index(name)
    rng = np.random.default_rng(500 + i)
    theta = float(rng.uniform(-0.6, 0.6))
    objects = []
    for o in range(n):
        objects.append({
            "shape": SHAPES[(i + o) % 3], "color": COLORS[(3 * i + o) % 8], "material": MATERIALS[(i + o) % 2],
            "size": SIZES[o % 2], "3d_coords": [float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), [0.35, 0.7][o % 2]],
            "pixel_coords": [int(rng.integers(20, 460)), int(rng.integers(20, 300)), float(rng.uniform(7, 14))],
            "rotation": float(rng.uniform(0, 360))})
    return {"image_index": 10 + i, "image_filename": "CLEVR_%s_%06d.png" % (split, 10 + i), "split": split, "objects": objects,
            "relationships": {k: [list(l) for l in v] for k, v in rel.items()},
            "directions": {"right": [float(np.cos(theta)), float(np.sin(theta)), 0.0], "above": [0.0, 0.0, 1.0]}}


def rows_of(name):
    """int64 (R,3): the rows [o2, pred, o1] of a case as extract_triplets lists them (clevr_dialog.py:293-297)."""
    n, rel = SCENES[name]
    return np.asarray([[o2, PREDS[k], o1] for k in rel for o1 in range(n) for o2 in rel[k][o1]], np.int64).reshape(-1, 3)


def closure_bits(rows, n):
    """path(M) of the rows (all of one predicate) as n bit rows."""
    C = [0] * n
    for s, _, o in rows:
        C[s] |= 1 << o
    for i in range(n):
        for j in range(n):
            if j != i and C[j] >> i & 1:
                C[j] |= C[i]
    return C


def reduce_rows(rows, n, keep):
    """The rule of the module docstring for the listed rows of ONE predicate -> list of [s, p, o]."""
    rows = [[int(v) for v in r] for r in rows]
    if len(rows) < 3:
        return rows
    M = [0] * n
    for s, _, o in rows:
        M[s] |= 1 << o
    H = closure_bits(rows, n)
    for j in range(n):
        old = H[j]
        self = old >> j & 1
        for i in range(n):
            if i == j:
                if self:
                    H[j] = 0
            elif H[i] >> j & 1 and (i < j or not self):
                H[i] &= ~old
    out = [h | m for h, m in zip(H, M)] if keep else H
    return [[s, rows[0][1], o] for s in range(n) for o in range(n) if out[s] >> o & 1]


def graph(rows, n, keep):
    """A sample's triplets (T,3) int64 from its listed rows: predicates in the order of their first rows, rows of
    __padding__ skipped, then the dummies."""
    rows = [r for r in np.asarray(rows).reshape(-1, 3).tolist() if r[1] != PREDS["__padding__"]]
    out = []
    for p in dict.fromkeys(r[1] for r in rows):
        out += reduce_rows([r for r in rows if r[1] == p], n, keep)
    out += [[i, PREDS["__in_image__"], n] for i in range(n)]
    return np.asarray(out, np.int64).reshape(-1, 3)


def padded_rows(names):
    """(rows int64 (B,R,3) padded with [0, __padding__, 0], n_objs (B,) = objects + 1) of a batch of cases."""
    rows = [rows_of(nm) for nm in names]
    R = max(len(r) for r in rows)
    out = np.zeros((len(names), R, 3), np.int64)
    out[..., 1] = PREDS["__padding__"]
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, np.asarray([SCENES[nm][0] + 1 for nm in names], np.int64)


def batch(rows, n_objs, keep):
    """The restatement of a padded batch -> (triplets (B,T,3), counts (B,))."""
    graphs = [graph(r, int(n) - 1, keep) for r, n in zip(rows, n_objs)]
    T = max(len(g) for g in graphs)
    out = np.zeros((len(graphs), T, 3), np.int64)
    out[..., 1] = PREDS["__padding__"]
    for b, g in enumerate(graphs):
        out[b, :len(g)] = g
    return out, np.asarray([len(g) for g in graphs], np.int64)


_GOLDEN = []


def golden():
    """(metadata, arrays) of tests/golden/clevr_unpacked.npz, read once."""
    if not _GOLDEN:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clevr_unpacked.npz")) as z:
            arrays = {k: z[k] for k in z.files if k != "__meta__"}
            _GOLDEN.append((json.loads(bytes(z["__meta__"]).decode()), arrays))
    return _GOLDEN[0]


def write_folder(root, split="train", dialog=True):
    """<root>/CLEVR/CLEVR_Dialog in the reference's layout with the four scenes of MIXED: scenes/CLEVR_<split>_scenes.json,
    seeded PNGs under images/<split>/ (RGBA and RGB), and the dialog file that names them.  -> base"""
    from PIL import Image
    base = os.path.join(root, "CLEVR", "CLEVR_Dialog")
    os.makedirs(os.path.join(base, "scenes"), exist_ok=True)
    os.makedirs(os.path.join(base, "images", split), exist_ok=True)
    scenes = [scene_dict(nm, split) for nm in MIXED]
    for i, (s, mode, (h, w)) in enumerate(zip(scenes, FOLDER_MODES, FOLDER_SIZES)):
        px = np.random.default_rng(90 + i).integers(0, 256, size=(h, w, len(mode)), dtype=np.uint8)
        Image.fromarray(px, mode).save(os.path.join(base, "images", split, s["image_filename"]))
    with open(os.path.join(base, "scenes", "CLEVR_%s_scenes.json" % split), "w") as f:
        json.dump({"info": {"split": split}, "scenes": scenes}, f)
    if dialog:
        with open(os.path.join(base, "clevr_dialog_%s_raw.json" % split), "w") as f:
            json.dump([{"split": split, "image_filename": s["image_filename"], "dialogs": []} for s in scenes], f)
    return base
