"""The Visual Genome input stage's cases and host restatements (tests/test_vg_cases.py pins them on the CPU,
tests/test_gpu_vg.py holds csrc/vg.hip and the folder dataset to them bit for bit).

`rows_fp64` restates csg_vg_rows: the per-object loop of the reference's __getitem__ (sg2im/data/packed_vg.py:110-125) and
the collate's padding (:186-205) in numpy fp64, rounded once to fp32.  tests/golden/vg_samples.npz holds what the reference
itself made of small seeded tables (tests/golden/make_golden_vg.py); `write_folder` writes those tables as a folder in the
reference's layout, with the split file as .npz."""
import json
import os
import random

import numpy as np

import preprocess_cases as pc
from conftest import load_golden

MEAN = STD = (0.5, 0.5, 0.5)
TABLES = ("object_names", "object_boxes", "objects_per_image", "relationship_subjects", "relationship_predicates",
          "relationship_objects", "relationships_per_image")
# the pictures of the folder, by sample: file name (the stem is the image id) and the mode it is saved in
FOLDER_FILES = ["VG_100K/100.png", "VG_100K/101.png", "VG_100K_2/2317.png", "VG_100K_2/7.jpg"]
FOLDER_MODES = ["RGB", "L", "RGBA", "RGB"]

_GOLDEN = []


def golden():
    """(meta, {key: numpy array}) of tests/golden/vg_samples.npz: read once, shared, never written to."""
    if not _GOLDEN:
        meta, g = load_golden("vg_samples")
        arrays = {k: v.numpy() for k, v in g.items()}
        for a in arrays.values():
            a.setflags(write=False)
        _GOLDEN.append((meta, arrays))
    return _GOLDEN[0]


def setting_id(si):
    s = golden()[0]["settings"][si]
    return "max%d_orphans%d_rels%d_trans%d" % (s["max_objects"], s["use_orphaned_objects"], s["include_relationships"],
                                               s["learned_transitivity"])


def vocab():
    """The golden's vocabulary as a vocab.json holds it: no `attributes`, the dataset adds them."""
    from canonicalsg2im_amd.synth import make_vocab
    v = make_vocab("vg")
    return {k: v[k] for k in ("object_name_to_idx", "object_idx_to_name", "pred_name_to_idx", "pred_idx_to_name")}


def rows_fp64(rows, sizes, counts, num_names):
    """rows (B,O,5) int = name, x, y, w, h; sizes (B,2) = HH, WW; counts (B,) -> (objs int64 (B,O), boxes fp32 (B,O,4)):
    objs = name and box = (x / WW, y / HH, w / WW, h / HH) in fp64, rounded once; 0 and -1 at or beyond the count, and in a
    row whose name is outside 1 .. num_names - 1 or whose picture has a side below 1 (the device's stale-row rule)."""
    rows = np.asarray(rows, np.int64)
    sizes = np.asarray(sizes, np.int64)
    B, O = rows.shape[:2]
    real = np.arange(O)[None] < np.asarray(counts)[:, None]
    real &= (rows[..., 0] >= 1) & (rows[..., 0] < num_names) & (sizes[:, None, 0] >= 1) & (sizes[:, None, 1] >= 1)
    HH = sizes[:, None, 0].astype(np.float64)
    WW = sizes[:, None, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.stack([rows[..., 1].astype(np.float64) / WW, rows[..., 2].astype(np.float64) / HH,
                      rows[..., 3].astype(np.float64) / WW, rows[..., 4].astype(np.float64) / HH], -1)
    boxes = np.where(real[..., None], q, -1.0).astype(np.float32)
    return np.where(real, rows[..., 0], 0).astype(np.int64), boxes


def padded_rows(tables, samples, picks):
    """The chosen objects of every sample as the builder lays them out: rows (B,O,5) int32 = name, x, y, w, h with -1 in the
    padding rows, counts (B,) int64; O is the largest count."""
    counts = np.asarray([len(chosen) for chosen in picks], np.int64)
    rows = np.full((len(samples), max(int(counts.max()), 1), 5), -1, np.int32)
    for b, (i, chosen) in enumerate(zip(samples, picks)):
        rows[b, :len(chosen), 0] = tables["object_names"][i, chosen]
        rows[b, :len(chosen), 1:] = tables["object_boxes"][i, chosen]
    return rows, counts


def with_image_row(objs, boxes):
    """What the collate hands on: one more row, 0 / -1 — the __image__ row of the fullest sample; every other sample has its
    own at its count already, since __image__ and the padding are both 0 / -1."""
    B = objs.shape[0]
    return np.concatenate([objs, np.zeros((B, 1), np.int64)], 1), np.concatenate([boxes, -np.ones((B, 1, 4), np.float32)], 1)


def golden_annotated(g, si, b, vocab):
    """The annotated rows of sample b of setting si, recovered from the golden triplets: type 0, a predicate that is neither
    meta nor a location relation.  A set: add_learnt_triplets sorts and merges the rows (np.unique)."""
    t, tt = g["s%d_triplets" % si][b], g["s%d_tt" % si][b]
    plain = {i for i, name in enumerate(vocab["pred_idx_to_name"]) if not name.startswith("__")}
    return {tuple(int(v) for v in row) for row, kind in zip(t, tt) if kind == 0 and int(row[1]) in plain}


def select_all(ds, si, rng=random):
    """`ds.select` for the samples of setting si in order, after seeding the `random` module as the golden did."""
    s = golden()[0]["settings"][si]
    random.seed(s["seed"])
    return [ds.select(i, rng) for i in s["samples"]]


# ------------------------------------------------------------------------------- a tiny folder in the reference's layout
def folder_pixels(i):
    """The seeded picture of sample i in the mode it is saved in: uint8 (h, w) for L, (h, w, 3 | 4) otherwise."""
    h, w = (int(v) for v in golden()[1]["sizes"][i])
    mode = FOLDER_MODES[i]
    shape = (h, w) if mode == "L" else (h, w, len(mode))
    return np.random.default_rng(900 + i).integers(0, 256, size=shape, dtype=np.uint8)


def write_folder(root, split="train", paths_as_bytes=False, extra_predicate=False):
    """<root>/vg in the reference's layout (sg2im/data/dataset_params.py:40-60): images/<FOLDER_FILES> of the golden's sizes —
    an RGB PNG, an L-mode PNG, an RGBA PNG and a JPEG —, <split>.npz with the golden's tables under the names
    scripts/preprocess_packed_vg.py writes (plus a key the loader has to ignore), vocab.json.  extra_predicate: vocab.json
    gets one predicate more.  Returns (base, [the decoded RGB pixels of every picture, as Pillow decodes the file])."""
    from PIL import Image
    _, g = golden()
    base = os.path.join(root, "vg")
    decoded = []
    for i, (name, mode) in enumerate(zip(FOLDER_FILES, FOLDER_MODES)):
        path = os.path.join(base, "images", name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(folder_pixels(i), mode).save(path, **({"quality": 90} if name.endswith(".jpg") else {}))
        with Image.open(path) as im:
            assert im.mode == mode
            decoded.append(np.asarray(im.convert("RGB")))
    paths = np.asarray([p.encode() for p in FOLDER_FILES] if paths_as_bytes else FOLDER_FILES)
    np.savez(os.path.join(base, split + ".npz"), image_paths=paths, image_ids=np.arange(4),
             **{k: g[k] for k in TABLES})
    v = vocab()
    if extra_predicate:
        v["pred_name_to_idx"]["one more"] = len(v["pred_idx_to_name"])
        v["pred_idx_to_name"] = v["pred_idx_to_name"] + ["one more"]
    with open(os.path.join(base, "vocab.json"), "w") as f:
        json.dump(v, f)
    return base, decoded


def to_float(u8):
    return pc.to_float(u8, mean=MEAN, std=STD)
