"""The unpacked Visual Genome dataset's cases and host restatements (tests/test_vg_unpacked_cases.py pins them on the CPU,
tests/test_gpu_vg_unpacked.py holds csrc/canon_small.hip and the folder dataset to them; equality everywhere).

`annotated_graph` restates the box-free graph of sg2im/data/vg.py:136-149: the annotated rows and the __in_image__ dummies
through add_learnt_triplets (sg2im/data/base_dataset.py:89-151), with oracle/canon.py's `path` and `choice_cdf`.
tests/golden/vg_unpacked.npz holds what the reference itself made of small seeded tables
(tests/golden/make_golden_vg_unpacked.py); `write_folder` writes those tables as a folder in the reference's layout."""
import copy
import json
import os
import random

import numpy as np

from conftest import load_golden
from oracle.canon import ORIGINAL_EDGE, TRANSITIVE_EDGE, choice_cdf, path

TABLES = ("object_names", "object_boxes", "objects_per_image", "relationship_subjects", "relationship_predicates",
          "relationship_objects", "relationships_per_image")
_GOLDEN = []


def golden():
    """(meta, {key: numpy array}) of tests/golden/vg_unpacked.npz: read once, shared, never written to."""
    if not _GOLDEN:
        meta, g = load_golden("vg_unpacked")
        arrays = {k: v.numpy() for k, v in g.items()}
        for a in arrays.values():
            a.setflags(write=False)
        _GOLDEN.append((meta, arrays))
    return _GOLDEN[0]


def setting_id(si):
    s = golden()[0]["settings"][si]
    return "max%d_orphans%d_rels%d_trans%d_conv%d" % (s["max_objects"], s["use_orphaned_objects"], s["include_relationships"],
                                                      s["learned_transitivity"], s["learned_converse"])


def vocab_json():
    """The golden's vocabulary as its vocab.json holds it: no `attributes`, no `__padding__`, no location predicate."""
    return copy.deepcopy(golden()[0]["vocab_json"])


def dataset_vocab(v=None):
    """What the reference's constructor makes of a vocab.json (sg2im/data/vg.py:64-71)."""
    v = vocab_json() if v is None else copy.deepcopy(v)
    v["attributes"] = {"objects": v["object_name_to_idx"]}
    v["reverse_attributes"] = {a: {i: k for k, i in t.items()} for a, t in v["attributes"].items()}
    v["pred_name_to_idx"]["__padding__"] = len(v["pred_name_to_idx"])
    v["pred_idx_to_name"] = list(v["pred_idx_to_name"]) + ["__padding__"]
    return v


def annotated_graph(objs0, rows, vocab, learned_transitivity=False, include_dummies=True, learned_converse=False,
                    converse_weights=None, uniforms=None):
    """One sample: (triplets (T,3), triplet_type (T,), conv_counts (P,P+1) float64).  `rows` (R,3) are the annotated
    relationships in local object indices; `uniforms` an iterator over the numbers of the converse draws.  A sample whose
    objects hold no __image__ id gets no dummies (the reference raises there; the kernels' rule)."""
    objs0 = np.asarray(objs0)
    O = objs0.shape[0]
    p2i = vocab["pred_name_to_idx"]
    n_rel = len(p2i)
    image_id = vocab["object_name_to_idx"]["__image__"]
    parts = [np.asarray(rows, np.int64).reshape(-1, 3)]                       # vg.py:136-146
    at = np.nonzero(objs0 == image_id)[0]
    if include_dummies and len(at):                                           # base_dataset.py:141-151
        img = int(at[0])
        others = np.array([i for i in range(O) if i != img], np.int64)
        parts.append(np.stack([others, np.full_like(others, p2i["__in_image__"]), np.full_like(others, img)], axis=1))
    trip = np.unique(np.concatenate(parts, axis=0).astype(np.int64), axis=0)  # :90
    meta = {p2i["__padding__"], p2i["__in_image__"]}
    non_meta = sorted(set(p2i.values()) - meta)
    conv_counts = np.zeros((n_rel, n_rel + 1))
    new = []
    for rel in non_meta:                                                      # :98-109
        rel_t = trip[trip[:, 1] == rel]
        if not len(rel_t):
            continue
        new.extend(rel_t.tolist())
        if learned_converse:                                                  # graphs_utils.py:130-155
            cands = [c for c in non_meta if c != rel]
            cdf = choice_cdf(converse_weights, rel, cands)
            vals = cands + [n_rel]
            for t in rel_t:
                r = vals[int(np.searchsorted(cdf, next(uniforms), side="right"))]
                conv_counts[rel, r] += 1
                if r != n_rel:
                    new.append([int(t[2]), r, int(t[0])])
    extra = []
    if learned_transitivity and new:                                          # :111-121, graphs_utils.py:101-105
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
    for rel in sorted(meta):                                                  # :123-126
        new.extend(trip[trip[:, 1] == rel].tolist())
    out = np.unique(np.asarray(new, np.int64).reshape(-1, 3), axis=0)         # :129-130
    ttype = [ORIGINAL_EDGE] * len(out)
    if extra:
        extra = np.concatenate(extra, axis=0).astype(np.int64)
        out = np.concatenate([out, extra], axis=0)
        ttype += [TRANSITIVE_EDGE] * len(extra)
    return out, np.asarray(ttype, np.int64), conv_counts


def annotated_batch(objs0, n_objs, rel, vocab, learned_transitivity=False, include_dummies=True, learned_converse=False,
                    converse_weights=None, uniforms=None):
    """Padded batch as vg_collate_fn pads it (vg.py:214-219): triplets (B,T,3) with [0, __padding__, 0], triplet_type (B,T)
    with 0, per-sample counts and conv_counts (B,P,P+1) float32.  `rel` (B,R,3): annotated rows, padding rows carry
    __padding__.  The samples consume `uniforms` one after the other."""
    pad = vocab["pred_name_to_idx"]["__padding__"]
    it = iter(uniforms) if uniforms is not None else None
    outs, convs = [], []
    for b in range(len(n_objs)):
        n = int(n_objs[b])
        rows = np.asarray(rel[b]).reshape(-1, 3)
        t, tt, cc = annotated_graph(objs0[b][:n], rows[rows[:, 1] != pad], vocab, learned_transitivity, include_dummies,
                                    learned_converse, converse_weights, it)
        outs.append((t, tt))
        convs.append(cc)
    T = max([len(t) for t, _ in outs] + [0])
    B = len(outs)
    trip = np.zeros((B, T, 3), np.int64)
    trip[:, :, 1] = pad
    ttype = np.zeros((B, T), np.int64)
    counts = np.zeros(B, np.int64)
    for b, (t, tt) in enumerate(outs):
        trip[b, :len(t)] = t
        ttype[b, :len(t)] = tt
        counts[b] = len(t)
    return trip, ttype, counts, np.stack(convs).astype(np.float32)


def draw_count(rel, vocab):
    """The converse draws of a batch: every sample's distinct rows of non-meta predicates."""
    p2i = vocab["pred_name_to_idx"]
    total = 0
    for rows in np.asarray(rel):
        rows = rows[(rows[:, 1] != p2i["__padding__"]) & (rows[:, 1] != p2i["__in_image__"])]
        total += len(np.unique(rows, axis=0)) if len(rows) else 0
    return total


def golden_conv(g, si, B, P):
    """conv_counts (B,P,P+1) float32 of setting si, dense (zeros without learned_converse)."""
    conv = np.zeros((B * P, P + 1), np.float32)
    if "s%d_conv_rows" % si in g:
        conv[g["s%d_conv_rows" % si]] = g["s%d_conv_vals" % si]
    return conv.reshape(B, P, P + 1)


def select_all(ds, si, rng=random):
    """`ds.select` for the samples of setting si in order, after seeding the `random` module as the golden did."""
    s = golden()[0]["settings"][si]
    random.seed(s["seed"])
    return [ds.select(i, rng) for i in s["samples"]]


def padded_rel(picks, pad):
    """The annotated rows of every sample as the builder lays them out: (B,R,3) int64, [0, __padding__, 0] beyond a sample's."""
    R = max(len(rows) for _, rows in picks)
    rel = np.zeros((len(picks), R, 3), np.int64)
    rel[:, :, 1] = pad
    for b, (_, rows) in enumerate(picks):
        if rows:
            rel[b, :len(rows)] = rows
    return rel


# ------------------------------------------------------------------------------- a tiny folder in the reference's layout
def write_folder(root, split="train"):
    """<root>/VisualGenome in the reference's layout (sg2im/data/dataset_params.py:110-127): the pictures of the golden's sizes
    at its image_paths (tiny seeded RGB PNGs), <split>.npz with the golden's tables, vocab.json.  Returns the base path."""
    from PIL import Image
    meta, g = golden()
    base = os.path.join(root, "VisualGenome")
    for i, name in enumerate(meta["image_paths"]):
        h, w = (int(v) for v in g["sizes"][i])
        where = os.path.join(base, name)
        os.makedirs(os.path.dirname(where), exist_ok=True)
        Image.fromarray(np.random.default_rng(700 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB").save(where)
    np.savez(os.path.join(base, split + ".npz"), image_paths=np.asarray(meta["image_paths"]), **{k: g[k] for k in TABLES})
    with open(os.path.join(base, "vocab.json"), "w") as f:
        json.dump(meta["vocab_json"], f)
    return base


# ------------------------------------------------------------------------------- the small-graph kernel's cases
B, O = 3, 64


def build_cases(vocab, seed=5):
    """{name: dict(objs, n, rel, include_dummies)} — the ten graphs of the issue's table, three samples each (B = 3, O = 64)."""
    p2i = vocab["pred_name_to_idx"]
    P, pad, in_image = len(p2i), p2i["__padding__"], p2i["__in_image__"]
    plain = [p for p in range(P) if p not in (pad, in_image)]
    last = max(plain)                                        # P - 1 unless a meta predicate sits there
    rng = np.random.default_rng(seed)
    num_objects = len(vocab["object_idx_to_name"])

    def sample(n, with_image=True):
        objs = np.zeros(O, np.int64)
        if n:
            objs[:n] = rng.integers(1, num_objects, n)
            if with_image:
                objs[n - 1] = 0
        return objs

    def random_rows(n, k):
        if n < 2 or k == 0:
            return []
        return [[int(rng.integers(0, n)), int(rng.choice(plain[:3] if len(plain) >= 3 else plain)), int(rng.integers(0, n))]
                for _ in range(k)]

    def batch(samples, dummies=True):
        n = np.asarray([s[0] for s in samples], np.int64)
        objs = np.stack([s[1] for s in samples])
        R = max([len(s[2]) for s in samples] + [1])
        rel = np.zeros((B, R, 3), np.int64)
        rel[:, :, 1] = pad
        for b, s in enumerate(samples):
            if s[2]:
                rel[b, :len(s[2])] = s[2]
        return {"objs": objs, "n": n, "rel": rel, "include_dummies": dummies}

    def filler(n):
        return (n, sample(n), random_rows(n, 2 * n))

    p0 = plain[0]
    cases = {}
    # 1: n = 64 and rows touching object 63 (bit 63 of a word, the last lane); 62 -> 63 -> 0 chains through it
    rows = random_rows(64, 40) + [[63, p0, 0], [62, p0, 63], [63, last, 63], [0, last, 63], [5, p0, 62]]
    cases["n64_object63"] = batch([(64, sample(64), rows), filler(9), filler(33)])
    # 2: n = 1, __image__ alone
    cases["image_alone"] = batch([filler(7), (1, sample(1), []), filler(20)])
    # 3: a sample with no annotated row
    cases["no_rows"] = batch([(12, sample(12), []), filler(5), (30, sample(30), [])])
    # 4: duplicated rows and self-relations
    rows = [[1, p0, 2], [1, p0, 2], [2, p0, 2], [3, p0, 3], [2, p0, 4], [1, p0, 2], [4, last, 4], [4, last, 4]]
    cases["duplicates_self"] = batch([(6, sample(6), rows), filler(11), (6, sample(6), rows[::-1])])
    # 5: a chain 0 -> 1 -> ... -> 62 of one predicate: the longest closure, 62 * 61 / 2 = 1891 extras
    chain = [[i, p0, i + 1] for i in range(62)]
    cases["chain"] = batch([filler(4), (64, sample(64), chain), (64, sample(64), [r for r in reversed(chain)][:40])])
    # 6: a cycle (path() then marks i -> i), and two cycles that share an object
    cyc = [[i, p0, (i + 1) % 7] for i in range(7)]
    two = [[0, last, 1], [1, last, 0], [1, last, 2], [2, last, 1], [9, last, 9]]
    cases["cycle"] = batch([(8, sample(8), cyc), (10, sample(10), two), (64, sample(64), [[i, p0, (i + 1) % 63] for i in range(63)])])
    # 7: a predicate with the largest id
    rows = [[0, last, 1], [1, last, 2], [2, last, 3], [0, p0, 3]]
    cases["last_predicate"] = batch([(5, sample(5), rows), filler(17), (3, sample(3), [[0, last, 1]])])
    # 8: __in_image__ rows given as annotations, some repeating a dummy, some not one
    rows = [[0, in_image, 4], [1, in_image, 4], [2, in_image, 0], [4, in_image, 4], [0, p0, 1]]
    cases["in_image_given"] = batch([(5, sample(5), rows), filler(8), (5, sample(5), rows[:2])])
    # 9: include_dummies off
    cases["no_dummies"] = batch([filler(10), (4, sample(4), [[0, in_image, 3], [0, p0, 1]]), (9, sample(9), [])], dummies=False)
    # 10: a sample whose objects contain no __image__ id, and one that has it twice (the first counts)
    twice = sample(9)
    twice[3] = 0
    cases["no_image_id"] = batch([(6, sample(6, with_image=False), random_rows(6, 9)), (9, twice, random_rows(9, 12)), filler(12)])
    for c in cases.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return cases


def converse_operands(vocab, rel, seed=3):
    """(weights (P,P) float32, uniforms float64) for the converse draws of `rel`: seeded uniforms, of which one is exactly a
    threshold of the first drawn relation's cdf and one lies in "none" (at or above the last candidate's threshold)."""
    p2i = vocab["pred_name_to_idx"]
    P, pad, in_image = len(p2i), p2i["__padding__"], p2i["__in_image__"]
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(P, P)).astype(np.float32)
    w = np.triu(w) + np.triu(w).T
    total = draw_count(rel, vocab)
    u = rng.random(total + 4)
    non_meta = [p for p in range(P) if p not in (pad, in_image)]
    first = None
    for rows in np.asarray(rel):                             # the first draw is of the first sample's lowest drawn predicate
        rows = rows[(rows[:, 1] != pad) & (rows[:, 1] != in_image)]
        if len(rows):
            first = int(rows[:, 1].min())
            break
    if first is not None and total >= 2:
        cdf = choice_cdf(w, first, [c for c in non_meta if c != first])
        u[0] = cdf[0] if len(cdf) > 1 else 0.5               # exactly a threshold: searchsorted(side="right") steps past it
        u[1] = np.nextafter(1.0, 0.0)                        # "none"
    return w, u
