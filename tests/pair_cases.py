"""The sampled-pair graph's cases and host restatements (tests/test_pair_cases.py pins them on the CPU,
tests/test_gpu_coco_pairs.py holds csg_pair_relations, csg_canon_general_build_dev and the `coco` folder dataset to them).

`pair_rows_atan2` restates the reference's loop (sg2im/data/coco.py:372-421) for one sample: the boxes and centres are fp32
values, every sum and difference is rounded to fp32 as the reference's tensors round it, and the angle is Python's
math.atan2 in double against multiples of math.pi / 4 — really called, not restated.  `sector_by_comparison` is the rule
csg_pair_relations decides by instead; both are compared over `tie_pairs()`.  `graph_from_rows` is the rest of the graph
(add_dummy_triplets, add_learnt_triplets, sg2im/data/base_dataset.py:89-151) on oracle/canon.py's `path` and `choice_cdf`.
tests/golden/coco_pairs.npz holds what the reference itself made (tests/golden/make_golden_coco.py); `write_folder` writes
its first group as a folder in the reference's layout."""
import json
import math
import os

import numpy as np

from conftest import load_golden
from oracle.canon import ORIGINAL_EDGE, TRANSITIVE_EDGE, choice_cdf, path

LEFT, ABOVE, RIGHT, BELOW = "__left of__", "__above__", "__right of__", "__below__"
f32 = np.float32
_GOLDEN = []


def golden():
    """(meta, {key: numpy array}) of tests/golden/coco_pairs.npz: read once, shared, never written to."""
    if not _GOLDEN:
        meta, g = load_golden("coco_pairs")
        arrays = {k: v.numpy() for k, v in g.items()}
        for a in arrays.values():
            a.setflags(write=False)
        _GOLDEN.append((meta, arrays))
    return _GOLDEN[0]


def vocab():
    """The golden's vocabulary, as the dataset builds it from the annotation files `write_folder` writes."""
    meta = golden()[0]
    n2i = dict(meta["object_name_to_idx"])
    names = ["NONE"] * (1 + max(n2i.values()))
    for name, idx in n2i.items():
        names[idx] = name
    return {"object_name_to_idx": n2i, "object_idx_to_name": names, "pred_name_to_idx": dict(meta["pred_name_to_idx"]),
            "pred_idx_to_name": list(meta["pred_idx_to_name"]), "attributes": {"objects": n2i},
            "reverse_attributes": {"objects": {v: k for k, v in n2i.items()}}}


def setting_id(si):
    s = golden()[0]["settings"][si]
    return "conv%d_trans%d_rels%d_lconv%d" % (s["use_converse"], s["learned_transitivity"], s["include_relationships"],
                                              s["learned_converse"])


def cases():
    """Every (setting, group) of the golden file."""
    return [(si, gi) for si, s in enumerate(golden()[0]["settings"]) for gi in range(len(s["groups"]))]


def case_id(case):
    return "%s_g%d" % (setting_id(case[0]), case[1])


def case_arrays(si, gi):
    """The arrays of one (setting, group), integers as int64, with the setting and the group's metadata."""
    meta, g = golden()
    tag = "s%d_g%d_" % (si, gi)
    out = {k[len(tag):]: (v if v.dtype == np.float32 else v.astype(np.int64)) for k, v in g.items() if k.startswith(tag)}
    out["other"], out["flip"] = out["other"].astype(np.int32), out["flip"].astype(np.uint8)
    out["n"] = g["counts"][meta["settings"][si]["groups"][gi]["samples"]]            # real objects per sample
    out["conv"] = out["conv"].astype(np.float32)
    if "s%d_weights" % si in g:
        out["weights"] = g["s%d_weights" % si]
    return meta["settings"][si], meta["settings"][si]["groups"][gi], out


def centers_of(boxes):
    """x0 + 0.5 * w, y0 + 0.5 * h in fp32: the reference's fallback for an empty mask (coco.py:356-358) and collate.py's."""
    boxes = np.asarray(boxes, f32)
    return (boxes[..., :2] + f32(0.5) * boxes[..., 2:]).astype(f32)


# ---------------------------------------------------------------------------------------------------- the two sector rules
def sector_by_atan2(dx, dy):
    """coco.py:387, :394-401: math.atan2 in double of the fp32 differences against multiples of math.pi / 4."""
    theta = math.atan2(float(dy), float(dx))
    if theta >= 3 * math.pi / 4 or theta <= -3 * math.pi / 4:
        return LEFT
    if -3 * math.pi / 4 <= theta < -math.pi / 4:
        return ABOVE
    if -math.pi / 4 <= theta < math.pi / 4:
        return RIGHT
    if math.pi / 4 <= theta < 3 * math.pi / 4:
        return BELOW
    raise AssertionError("no sector for theta = %r" % theta)


def sector_by_comparison(dx, dy):
    """The rule of csg_pair_relations: exact comparisons of fp32 values, no angle."""
    dx, dy = f32(dx), f32(dy)
    ax, ay, neg = abs(dx), abs(dy), bool(np.signbit(dx))
    if neg and ay <= ax:
        return LEFT
    if not neg and (ay < ax or (ay == ax and dy <= 0)):
        return RIGHT
    return ABOVE if dy < 0 else BELOW


def tie_pairs(seed=0, n_random=2000):
    """fp32 (dx, dy) pairs: seeded random differences, exact ties |dy| == |dx| in all four sign combinations with their
    one-ulp neighbours, denormals, and both signed zeros in both places."""
    rng = np.random.default_rng(seed)
    out = [(f32(a), f32(b)) for a, b in rng.uniform(-1, 1, size=(n_random, 2))]
    mags = [f32(0.25), f32(1.0), f32(1 / 3), f32(0.7), f32(1e-3), f32(3e-39), np.finfo(f32).tiny, f32(1.4e-45), f32(123.456)]
    mags += [f32(v) for v in rng.uniform(1e-6, 2, size=40)]
    for a in mags:
        near = [a, np.nextafter(a, f32(np.inf)), np.nextafter(a, f32(0))]
        for x in near:
            for y in near:
                for sx in (1, -1):
                    for sy in (1, -1):
                        out.append((f32(sx) * x, f32(sy) * y))
    zeros = [f32(0.0), f32(-0.0)]
    for z in zeros:
        for w in zeros + [f32(0.25), f32(-0.25), f32(1.4e-45), f32(-1.4e-45)]:
            out += [(z, w), (w, z)]
    return out


# ---------------------------------------------------------------------------------------------------- the reference's loop
def pair_rows_atan2(boxes, centers, n, other, flip, p2i, use_converse=False):
    """coco.py:372-421 for one sample with `n` real objects: rows [[s, p, o]] for cur = 0 .. n - 1, or [] when nothing was
    drawn (other[0] < 0).  fp32 in, fp32 sums and differences, math.atan2 in double."""
    boxes, centers = np.asarray(boxes, f32), np.asarray(centers, f32)
    rows = []
    for cur in range(n if n >= 2 and other[0] >= 0 else 0):
        s, o = (int(other[cur]), cur) if flip[cur] else (cur, int(other[cur]))
        sx0, sy0, sw, sh = boxes[s]
        ox0, oy0, ow, oh = boxes[o]
        sx1, sy1 = f32(sx0 + f32(sw / f32(2))), f32(sy0 + f32(sh / f32(2)))
        ox1, oy1 = f32(ox0 + f32(ow / f32(2))), f32(oy0 + f32(oh / f32(2)))
        d = (centers[s] - centers[o]).astype(f32)
        if sx0 < ox0 and sx1 > ox1 and sy0 < oy0 and sy1 > oy1:
            p = "__surrounding__"
        elif sx0 > ox0 and sx1 < ox1 and sy0 > oy0 and sy1 < oy1:
            p = "__inside__"
        else:
            p = sector_by_atan2(d[0], d[1])
        if use_converse and p in ("__inside__", RIGHT, BELOW):                       # :404-421
            p = {"__inside__": "__surrounding__", RIGHT: LEFT, BELOW: ABOVE}[p]
            s, o = o, s
        rows.append([s, p2i[p], o])
    return rows


def padded_rows(rows_per_sample, O, p2i):
    out = np.zeros((len(rows_per_sample), O, 3), np.int64)
    out[:, :, 1] = p2i["__padding__"]
    for b, rows in enumerate(rows_per_sample):
        if rows:
            out[b, :len(rows)] = rows
    return out


# ---------------------------------------------------------------------------------------------------- the rest of the graph
def graph_from_rows(rows, n, vocab, learned_transitivity=False, learned_converse=False, converse_weights=None,
                    uniforms=None):
    """add_dummy_triplets + add_learnt_triplets (base_dataset.py:89-151) for one sample of `n` real objects whose
    __image__ row is row n -> (triplets (T,3), triplet_type (T,), conv_counts (P,P+1))."""
    p2i = vocab["pred_name_to_idx"]
    n_rel = len(p2i)
    parts = [np.asarray(rows, np.int64).reshape(-1, 3),
             np.asarray([[i, p2i["__in_image__"], n] for i in range(n)], np.int64).reshape(-1, 3)]
    trip = np.unique(np.concatenate(parts, axis=0), axis=0)
    meta = {p2i["__padding__"], p2i["__in_image__"]}
    non_meta = sorted(set(p2i.values()) - meta)
    conv_counts = np.zeros((n_rel, n_rel + 1))
    new = []
    for rel in non_meta:
        rel_t = trip[trip[:, 1] == rel]
        if not len(rel_t):
            continue
        new.extend(rel_t.tolist())
        if learned_converse:                                                      # graphs_utils.py:126-152
            cands = [c for c in non_meta if c != rel]
            cdf = choice_cdf(converse_weights, rel, cands)
            vals = cands + [n_rel]
            for t in rel_t:
                r = vals[int(np.searchsorted(cdf, next(uniforms), side="right"))]
                conv_counts[rel, r] += 1
                if r != n_rel:
                    new.append([int(t[2]), r, int(t[0])])
    extra = []
    if learned_transitivity and new:
        arr = np.asarray(new, np.int64)
        for rel in non_meta:
            rel_t = arr[arr[:, 1] == rel]
            if not len(rel_t):
                continue
            N = int(max(rel_t[:, 0].max(), rel_t[:, 2].max()) + 1)
            g = np.zeros((N, N), bool)
            g[rel_t[:, 0], rel_t[:, 2]] = True
            s, o = np.nonzero(path(g) & ~g)
            extra.append(np.stack([s, np.full_like(s, rel), o], axis=1))
    for rel in sorted(meta):
        new.extend(trip[trip[:, 1] == rel].tolist())
    out = np.unique(np.asarray(new, np.int64).reshape(-1, 3), axis=0)
    ttype = [ORIGINAL_EDGE] * len(out)
    if extra:
        extra = np.concatenate(extra, axis=0).astype(np.int64)
        out = np.concatenate([out, extra], axis=0)
        ttype += [TRANSITIVE_EDGE] * len(extra)
    return out, np.asarray(ttype, np.int64), conv_counts


def batch_from_rows(rows, counts, vocab, **kw):
    """The collate's padding (coco.py:517-522) over graph_from_rows of every sample; the samples consume `uniforms` one after
    the other -> (triplets (B,T,3), triplet_type (B,T), conv_counts (B,P,P+1) float32)."""
    pad = vocab["pred_name_to_idx"]["__padding__"]
    if kw.get("uniforms") is not None:
        kw["uniforms"] = iter(kw["uniforms"])
    outs = []
    for b, n in enumerate(counts):
        r = np.asarray(rows[b]).reshape(-1, 3)
        outs.append(graph_from_rows(r[r[:, 1] != pad], int(n), vocab, **kw))
    T = max(len(t) for t, _, _ in outs)
    trip = np.zeros((len(outs), T, 3), np.int64)
    trip[:, :, 1] = pad
    ttype = np.zeros((len(outs), T), np.int64)
    for b, (t, tt, _) in enumerate(outs):
        trip[b, :len(t)] = t
        ttype[b, :len(t)] = tt
    return trip, ttype, np.stack([c for _, _, c in outs]).astype(np.float32)


def golden_uniforms(group, total):
    """The numbers the reference's np.random.choice consumed for a learned-converse group: one random_sample per draw."""
    state = np.random.get_state()
    np.random.seed(group["seed"])
    u = np.random.random_sample(total)
    np.random.set_state(state)
    return u


# ---------------------------------------------------------------------------------------------------- hand-written pairs
def hand_written():
    """(boxes fp32 (2,4), what it is about): two-object samples beyond the golden ones."""
    e = np.nextafter(f32(0.25), f32(1))
    return [
        (np.asarray([[0.25, 0.25, 0.25, 0.25], [e, 0.5, 0.25, 0.25]], f32), "one ulp right of the (+a,+a) tie"),
        (np.asarray([[0.25, 0.25, 0.25, 0.25], [0.5, e, 0.25, 0.25]], f32), "one ulp below the (+a,+a) tie"),
        (np.asarray([[0.1, 0.1, 0.6, 0.6], [0.2, 0.2, 0.2, 0.2]], f32), "surrounding by the reference's test"),
        (np.asarray([[0.1, 0.1, 0.6, 0.6], [0.2, 0.2, 0.4, 0.4]], f32), "corners surround, centres tie: not surrounding"),
        (np.asarray([[0.1, 0.1, 0.6, 0.6], [0.2, 0.05, 0.2, 0.2]], f32), "x surrounds, y does not"),
        (np.asarray([[0.3, 0.3, 0.1, 0.1], [0.3, 0.3, 0.1, 0.1]], f32), "identical boxes: d = (0, 0)"),
        (np.asarray([[0.0, 0.5, 0.1, 0.1], [0.9, 0.5, 0.1, 0.1]], f32), "far left / right, dy = 0"),
        (np.asarray([[0.5, 0.0, 0.1, 0.1], [0.5, 0.9, 0.1, 0.1]], f32), "far above / below, dx = 0"),
        (np.asarray([[1 / 3, 1 / 7, 1 / 9, 1 / 11], [1 / 5, 1 / 3, 1 / 13, 1 / 6]], f32), "inexact quotients"),
    ]


# ---------------------------------------------------------------------------------------------------- the folder
FOLDER_GROUP = 0


def folder_pixels(i):
    """The decoded picture of golden sample i: seeded noise of the recorded size."""
    h, w = golden()[1]["sizes"][i].tolist()
    return np.random.default_rng(40 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def write_folder(root, split="train", samples=None):
    """The golden's first group as <root>/MSCoco in the reference's layout: PNG pictures and the two annotation files
    (instances first, then stuff, as the golden rows are ordered) -> (image dir, [decoded pixels])."""
    from PIL import Image
    meta, g = golden()
    samples = meta["settings"][0]["groups"][FOLDER_GROUP]["samples"] if samples is None else samples
    base = os.path.join(root, "MSCoco")
    image_dir = os.path.join(base, "images", "%s2017" % split)
    os.makedirs(image_dir, exist_ok=True)
    os.makedirs(os.path.join(base, "annotations"), exist_ok=True)
    instance_ids = {c[0] for c in meta["instance_categories"]}
    images, ann, decoded = [], {"instances": [], "stuff": []}, []
    for i in samples:
        image_id = int(g["image_ids"][i])
        h, w = g["sizes"][i].tolist()
        name = "%012d.png" % image_id
        px = folder_pixels(i)
        Image.fromarray(px, "RGB").save(os.path.join(image_dir, name))
        decoded.append(px)
        images.append({"id": image_id, "file_name": name, "width": w, "height": h})
        for k in range(int(g["counts"][i])):
            cat = int(g["cats"][i, k])
            ann["instances" if cat in instance_ids else "stuff"].append(
                {"id": image_id * 100 + k, "image_id": image_id, "category_id": cat,
                 "bbox": [float(v) for v in g["boxes_px"][i, k]], "segmentation": []})
    for kind in ("instances", "stuff"):
        with open(os.path.join(base, "annotations", "%s_%s2017.json" % (kind, split)), "w") as f:
            json.dump({"images": images, "categories": [{"id": c[0], "name": c[1]} for c in meta["%s_categories" % kind[:-1]
                                                        if kind == "instances" else "stuff_categories"]],
                       "annotations": ann[kind]}, f)
    return image_dir, decoded
