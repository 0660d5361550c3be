"""The canonical-graph builders' case matrix: scene families, the table of rows and the expected values
(tests/test_canon_cases.py pins the families and the table on the CPU, tests/test_gpu_canon_paths.py holds csrc/canon.hip,
csrc/canon_small.hip and csrc/clevr_graph.hip to them; integers throughout: equality, no tolerance).

A ROW names a builder path, a scene family, the sizes of the samples of its one batch (rows per sample, the `__image__` row
included), where the `__image__` row sits, and the flags.  The paths, by the Python entry that serves them:
  lds           canonical_triplets, 8-predicate vocabulary, no `triplets`: k_canon_build / _converse / _emit
  general       canonical_triplets with `triplets=` (an empty (B,0,3) included) or a 46-predicate vocabulary: k_gen_*
  general_rows  canonical_triplets with boxes=None: the same kernels without geometry
  pairs         canonical_triplets with `pairs=`: k_pair_relations -> k_gen_pack -> k_gen_*
  small         canonical_triplets with boxes=None and a vocabulary without location predicates: annotated_triplets
  clevr         clevr_triplets
A row whose `paths` holds both lds and general is ONE scene served by both: the general path gets an empty `triplets`.

A FAMILY is a function of the number of real objects and a seed.  It writes float32 boxes and centres whose coordinates
are multiples of 2^-10 below 2, so every x0 + w / 2 and every difference of centres is exact: no comparison depends on a
rounding the family did not intend (`random` excepted: it is the generator the older tests use, kept for continuity).

The expected values come from the numpy restatements alone — oracle/canon.py, tests/canon_annotated.py,
tests/pair_cases.py, tests/vg_unpacked_cases.py, tests/clevr_graph_cases.py — which tests/golden/canon_structured.npz
(written by the reference itself, tests/golden/make_golden_canon_structured.py) pins on these families at small sizes."""
import copy
import itertools

import numpy as np

f32 = np.float32
D = f32(2.0 ** -10)

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)      # rows per sample, the __image__ row included
CHAIN_SIZES = (64, 65, 192, 193, 255, 256)                                # chains and `nested`: the oracle's cost is O(n^3)
LIMIT = {"lds": 256, "general": 256, "general_rows": 256, "pairs": 256, "small": 64, "clevr": 64}     # rows; clevr: 63 objects
REFUSAL = {"lds": "at most 256 objects", "general": "at most 256 objects", "general_rows": "at most 256 objects",
           "pairs": "at most 256 objects", "small": "at most 64 rows per sample", "clevr": "at most 63 objects per sample"}
BOX_PATHS = ("lds", "general", "pairs")
IMAGE_POSITIONS = ("last", "first", "middle", "absent", "twice")
MIXED = (256, 1, 193, 2, 64, 256, 3)
POISON_BOX, POISON_CENTRE = (-1.0, -1.0, 8.0, 8.0), (5.0, 5.0)           # surrounds every family's boxes; right of and below them


# ------------------------------------------------------------------------------------------------------- the families
def _ranked(rank):
    """Equal boxes on a diagonal: the object of rank r is left of and above every object of a higher rank."""
    rank = np.asarray(rank, np.int64)
    x = rank.astype(f32) * D
    boxes = np.stack([x, x, np.full_like(x, 2.0 ** -4), np.full_like(x, 2.0 ** -4)], 1).astype(f32)
    return boxes, (boxes[:, :2] + f32(2.0 ** -5)).astype(f32)


def fam_random(m, seed):
    """Uniform random boxes with three hand-placed ties: the generator of tests/test_gpu_canon.py."""
    rng = np.random.default_rng(seed)
    wh = rng.uniform(0.05, 0.6, size=(m, 2))
    xy = rng.uniform(0.0, 1.0, size=(m, 2)) * (1.0 - wh)
    if m >= 6:
        xy[1], wh[1] = xy[0], wh[0]
        xy[3, 0] = xy[2, 0]
        wh[5, 1] = wh[4, 1]
        xy[5, 1] = xy[4, 1]
    bx = np.concatenate([xy, wh], axis=1)
    return bx.astype(f32), np.stack([bx[:, 0] + 0.5 * bx[:, 2], bx[:, 1] + 0.5 * bx[:, 3]], axis=1).astype(f32)


def fam_chain(m, seed):
    """One total order on both axes, ascending with the index: every minimal edge links neighbours."""
    return _ranked(np.arange(m))


def fam_reverse_chain(m, seed):
    """The same order against the indices: Hsu's pivots and the (s, p, o) sort run against it."""
    return _ranked(np.arange(m)[::-1])


def fam_shuffled_chain(m, seed):
    return _ranked(np.random.default_rng(seed).permutation(m))


def fam_nested(m, seed):
    """Every pair is __inside__ / __surrounding__ by the reference's test, which compares x0 and x0 + w / 2 (the box CENTRE):
    the object of rank r spans [r d, 1 - r d] in those two, so concentric boxes would not do — the centres shift with r.
    Rank = index for an even seed, a seeded permutation otherwise."""
    rank = np.arange(m) if seed % 2 == 0 else np.random.default_rng(seed).permutation(m)
    x0 = rank.astype(f32) * D
    half = (f32(1.0) - f32(2.0) * x0).astype(f32)                           # x0 + half = 1 - r d
    boxes = np.stack([x0, x0, f32(2.0) * half, f32(2.0) * half], 1).astype(f32)
    return boxes, (boxes[:, :2] + half[:, None]).astype(f32)


def fam_identical(m, seed):
    """All boxes and centres equal: no location relation at all."""
    return np.tile(np.asarray([[0.25, 0.25, 0.5, 0.5]], f32), (m, 1)), np.full((m, 2), 0.5, f32)


def grid_side(m):
    return int(np.ceil(np.sqrt(max(m, 1))))


def fam_grid(m, seed):
    """k x k centres, filled row by row: k-way ties on each axis, so the orders are layered, not total."""
    k = grid_side(m)
    i = np.arange(m)
    x0, y0 = (i % k).astype(f32) * f32(2.0 ** -5), (i // k).astype(f32) * f32(2.0 ** -5)
    boxes = np.stack([x0, y0, np.full_like(x0, 2.0 ** -6), np.full_like(x0, 2.0 ** -6)], 1).astype(f32)
    return boxes, (boxes[:, :2] + f32(2.0 ** -7)).astype(f32)


def fam_two_clusters(m, seed, split=64, bridge=False, pivot_last=False):
    """A chain on objects 0 .. split-1 and another on split .. m-1 with no ordered pair between them: every object of the
    first cluster SURROUNDS every object of the second (the pair goes to __surrounding__ / __inside__, whose minimal graph
    is that full bipartite one), so the four order relations have edges inside the words and none across.  The centres
    ascend with the index over both clusters.  `bridge`: object `split` starts at x0 of object split-1, which therefore
    neither surrounds nor is inside it; that ONE pair is ordered, and the closure joins the clusters.  `pivot_last`: object
    split-1, through which every such path runs, changes places with the last object: where the `__image__` row is not the
    last one, Warshall's LAST pivot then makes all of them."""
    i = np.arange(m)
    first = i < split
    x0 = np.where(first, i.astype(f32) * D, f32(0.25) + i.astype(f32) * D).astype(f32)
    y0 = x0.copy()
    w = np.where(first, f32(1.75), f32(2.0 ** -4)).astype(f32)
    if bridge and m > split:
        x0[split] = f32(split - 1) * D
    boxes = np.stack([x0, y0, w, w], 1).astype(f32)
    c = i.astype(f32) * D
    cen = np.stack([c, c], 1).astype(f32)
    if pivot_last and m > split:
        swap = np.arange(m)
        swap[[split - 1, m - 1]] = m - 1, split - 1
        boxes, cen = boxes[swap], cen[swap]
    return boxes, cen


def fam_single(m, seed):
    assert m <= 1
    return fam_identical(m, seed)


FAMILIES = {"random": fam_random, "chain": fam_chain, "reverse_chain": fam_reverse_chain, "shuffled_chain": fam_shuffled_chain,
            "nested": fam_nested, "identical": fam_identical, "grid": fam_grid, "two_clusters": fam_two_clusters,
            "single": fam_single, "only_image": fam_single}


def image_rows(rows, image):
    """The indices of a sample's `__image__` rows."""
    return {"last": [rows - 1], "first": [0], "middle": [rows // 2], "absent": [], "twice": [rows // 2, rows - 1]}[image]


def sample(family, rows, seed, image="last", **kw):
    """One sample of `rows` rows -> (objs (rows,) int64, boxes (rows,4), centres (rows,2)).  The `__image__` rows (id 0) carry
    the poisoned box: only their id keeps them out of the pair loop."""
    at = image_rows(rows, image)
    assert len(set(at)) == len(at) and rows >= len(at)
    m = rows - len(at)
    fb, fc = FAMILIES[family](m, seed, **kw)
    objs = np.zeros(rows, np.int64)
    boxes = np.tile(np.asarray([POISON_BOX], f32), (rows, 1))
    cen = np.tile(np.asarray([POISON_CENTRE], f32), (rows, 1))
    real = np.asarray([i for i in range(rows) if i not in at], np.int64)
    objs[real] = 1 + (np.arange(m) + seed) % 3
    boxes[real], cen[real] = fb, fc
    return objs, boxes, cen


def annotated_rows(kind, m, vocab):
    """A sample's annotated relationships over m real objects (the __image__ row is row m).
    chain: one predicate along 0 -> 1 -> ... -> m-1 (across every word boundary the sample has), its first row given twice,
    and a two-cycle of another predicate (-> transitive self-loops); every other predicate has no row.
    every: each non-meta predicate of the vocabulary once."""
    p2i = vocab["pred_name_to_idx"]
    plain = sorted(set(p2i.values()) - {p2i["__padding__"], p2i["__in_image__"]})
    if m < 2:
        return []
    if kind == "chain":
        rows = [[i, plain[0], i + 1] for i in range(m - 1)]
        return rows + [rows[0], [0, plain[-1], 1], [1, plain[-1], 0]]
    assert kind == "every"
    return [[k % m, p, (k + 1) % m] for k, p in enumerate(plain)]


EVERY_AT = (2, 63, 128, 191)            # the samples (by rows) whose annotated rows are `every`; the others get `chain`


def pair_draws(kind, m, seed):
    """(other (m,) int32, flip (m,) uint8): every real object draws one other.  matching: i <-> i ^ 1; star: all draw
    object 0; cycle: i -> i + 1.  Nothing is drawn below two objects."""
    if m < 2:
        return np.full(m, -1, np.int32), np.zeros(m, np.uint8)
    i = np.arange(m)
    if kind == "matching":
        other = i ^ 1
        other[other >= m] = 0
    elif kind == "star":
        other = np.zeros(m, np.int64)
        other[0] = 1
    else:
        other = (i + 1) % m
    return other.astype(np.int32), ((i * 7 + seed) % 3 == 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- the table
def _row(id, paths, family, sizes, **kw):
    row = dict(id=id, paths=tuple(paths), family=family, sizes=tuple(sizes), seed=1, image="last", trans=0, dummies=1, conv=0,
               permuted=0, vocab="coco", annotated=False, pairs=None, use_converse=0, kw={}, refused=None, n_over=None, reversed=0)
    assert set(kw) <= set(row), kw
    row.update(kw)
    return row


def _table():
    flags = itertools.cycle(itertools.product((1, 0), (1, 0), (0, 1), (0, 1)))      # trans, dummies, conv, permuted

    def both(id, family, sizes, **kw):
        t, d, c, p = next(flags)
        if kw.get("image") in ("absent", "twice"):      # the restatement, like the reference, needs ONE __image__ row for dummies
            d = 0
        kw = dict(dict(trans=t, dummies=d, conv=c, permuted=p), **kw)
        return _row(id, ("lds", "general"), family, sizes, **kw)

    rows = [
        both("random_all", "random", SIZES),
        both("chain", "chain", CHAIN_SIZES, trans=1),
        both("reverse_chain", "reverse_chain", CHAIN_SIZES),
        both("shuffled_chain", "shuffled_chain", CHAIN_SIZES, seed=3),
        both("nested", "nested", CHAIN_SIZES, trans=1, seed=2),
        both("nested_shuffled", "nested", (65, 193), seed=5),
        both("identical", "identical", (3, 65, 256)),
        both("grid", "grid", (65, 129, 256), trans=1),
        both("two_clusters", "two_clusters", (129, 256)),
        both("two_clusters_bridge", "two_clusters", (129, 256), trans=1, kw={"bridge": True}),
        both("bridge_pivot_last", "two_clusters", (129, 256), trans=1, conv=0, image="absent", kw={"bridge": True, "pivot_last": True}),
        both("bridge_pivot_last_converse", "two_clusters", (129, 256), trans=1, conv=1, image="absent",
             kw={"bridge": True, "pivot_last": True}),
        both("single", "single", (2, 2)),
        both("only_image", "only_image", (1,)),
        both("mixed", "random", MIXED, seed=7, trans=1, conv=0, dummies=1, permuted=0),
        both("mixed_reversed", "random", MIXED[::-1], seed=7, trans=1, conv=0, dummies=1, permuted=0, reversed=1),
        both("image_first", "random", (12, 65, 256), image="first", seed=11),
        both("image_middle", "chain", (12, 65, 256), image="middle"),
        both("image_absent", "random", (12, 65, 256), image="absent", seed=12),
        both("image_twice", "shuffled_chain", (12, 65, 256), image="twice", seed=13),
        both("chain_converse", "chain", (65, 256), trans=1, conv=1),
        both("random_no_dummies", "random", (64, 129, 255), seed=17, dummies=0),
        both("grid_converse", "grid", (64, 192), seed=19, conv=1),
        both("nested_converse", "nested", (64, 193), seed=4, conv=1),
    ]
    # every (trans, dummies, conv, permuted) is on the lds path above: 32 rows over a cycle of 16, the last eight fix no flag
    rows += [both("flags_%d" % k, "random", (33, 66), seed=30 + k) for k in range(8)]
    rows += [
        _row("lds_n_over", ("lds", "general"), "random", (12, 65, 30), seed=21, conv=1, trans=1, n_over=(1, 66),
             refused=r"n_objs\[1\] = 66 outside \[0, 65\]"),
        _row("lds_257", ("lds", "general"), "chain", (3, 257), refused=REFUSAL["lds"]),
        # annotated rows over the geometry, 46 predicates
        _row("general_vg_all", ("general",), "random", SIZES, vocab="vg", annotated=True, trans=1, conv=1, seed=23),
        _row("general_vg_permuted", ("general",), "chain", (65, 256), vocab="vg", annotated=True, trans=1, permuted=1),
        _row("general_vg_no_rows", ("general",), "grid", (10, 129), vocab="vg", conv=1, dummies=0),
        # the rows alone
        _row("rows_all", ("general_rows",), "identical", SIZES, vocab="vg", annotated=True, trans=1, conv=1),
        _row("rows_plain", ("general_rows",), "identical", (2, 65, 256), vocab="vg", annotated=True, permuted=1),
        _row("rows_257", ("general_rows",), "identical", (3, 257), vocab="vg", annotated=True, refused=REFUSAL["general_rows"]),
        _row("rows_small_twin", ("general_rows", "small"), "identical", (1, 2, 3, 63, 64), vocab="vg", annotated=True, trans=1,
             conv=1),
        _row("small_all", ("small",), "identical", (1, 2, 3, 63, 64), vocab="vgu", annotated=True, trans=1, conv=1),
        _row("small_plain", ("small",), "identical", (64, 3), vocab="vgu", annotated=True, dummies=0),
        _row("small_65", ("small",), "identical", (3, 65), vocab="vgu", annotated=True, refused=REFUSAL["small"]),
        # the unpacked CLEVR dataset's rows: 63 objects are 64 rows with the __image__ row
        _row("clevr_all", ("clevr",), "shuffled_chain", (1, 2, 3, 4, 63, 64), vocab="clevr", seed=5),
        _row("clevr_keep", ("clevr",), "reverse_chain", (64, 4, 33), vocab="clevr", trans=1),
        _row("clevr_65", ("clevr",), "chain", (4, 65), vocab="clevr", refused=REFUSAL["clevr"]),
        # the sampled pairs: every real row draws
        _row("pairs_all", ("pairs",), "random", SIZES, pairs="cycle", trans=1, conv=1, seed=25),
        _row("pairs_matching", ("pairs",), "random", (255, 256, 3), pairs="matching", trans=1, use_converse=1, seed=26),
        _row("pairs_star", ("pairs",), "nested", (255, 256), pairs="star", trans=1, conv=1, seed=2),
        _row("pairs_cycle", ("pairs",), "chain", (255, 256), pairs="cycle", trans=1),
        _row("pairs_cycle_converse", ("pairs",), "reverse_chain", (256, 255), pairs="cycle", trans=1, use_converse=1, conv=1),
        _row("pairs_257", ("pairs",), "chain", (3, 257), pairs="cycle", refused=REFUSAL["pairs"]),
    ]
    for fam in FAMILIES:                               # every family on the pairs path as well
        if fam not in ("random", "nested", "chain", "reverse_chain"):
            kw = {"kw": {"bridge": True}} if fam == "two_clusters" else {}
            sizes = {"single": (2,), "only_image": (1,)}.get(fam, (65, 130))
            rows.append(_row("pairs_" + fam, ("pairs",), fam, sizes, pairs="matching", seed=3, **kw))
    return rows


TABLE = _table()
ROWS = {r["id"]: r for r in TABLE}
assert len(ROWS) == len(TABLE)


# ------------------------------------------------------------------------------------------------------- a row's inputs
_PERM8 = (3, 7, 1, 0, 6, 2, 5, 4)


def vocab_of(row):
    from canonicalsg2im_amd.synth import make_vocab
    if row["vocab"] == "vgu":                          # the unpacked Visual Genome's: no location predicate
        import vg_unpacked_cases as vu
        return vu.dataset_vocab()
    if row["vocab"] == "clevr":
        import clevr_graph_cases as gc
        return gc.golden()[0]["vocab"]
    vocab = copy.deepcopy(make_vocab(row["vocab"]))
    if row["permuted"]:
        names = list(vocab["pred_idx_to_name"])
        perm = _PERM8 if len(names) == 8 else np.random.default_rng(5).permutation(len(names))
        vocab["pred_idx_to_name"] = [names[i] for i in perm]
        vocab["pred_name_to_idx"] = {nm: i for i, nm in enumerate(vocab["pred_idx_to_name"])}
    return vocab


def inputs(row, O=None):
    """The padded batch of a row: objs (B,O) int64, boxes (B,O,4), centres (B,O,2), n (B,), and what the row's path needs
    besides (rel (B,R,3); other, flip (B,O); weights, uniforms).  Rows n <= row < O are poisoned: a box that surrounds every
    family's, a centre right of and below them, an object id that is not __image__."""
    sizes = row["sizes"]
    B = len(sizes)
    O = max(sizes) if O is None else O
    assert O >= max(sizes)
    vocab = vocab_of(row)
    p2i = vocab["pred_name_to_idx"]
    objs = np.ones((B, O), np.int64)
    boxes = np.tile(np.asarray(POISON_BOX, f32), (B, O, 1))
    cen = np.tile(np.asarray(POISON_CENTRE, f32), (B, O, 1))
    out = {"vocab": vocab, "n": np.asarray(sizes, np.int64)}
    for b, n in enumerate(sizes):
        k = B - 1 - b if row["reversed"] else b          # a reversed row holds the SAME samples, last first
        objs[b, :n], boxes[b, :n], cen[b, :n] = sample(row["family"], n, row["seed"] + k, row["image"], **row["kw"])
    out.update(objs=objs, boxes=boxes, centers=cen)
    if row["n_over"]:
        out["n"][row["n_over"][0]] = row["n_over"][1]
    if row["annotated"]:
        assert row["image"] == "last"
        rels = [annotated_rows("every" if n in EVERY_AT else "chain", n - 1, vocab) for n in sizes]
        R = max(len(r) for r in rels)
        rel = np.zeros((B, R, 3), np.int64)
        rel[:, :, 1] = p2i["__padding__"]
        for b, r in enumerate(rels):
            if r:
                rel[b, :len(r)] = r
        out["rel"] = rel
    if row["pairs"]:
        assert row["image"] == "last"
        other, flip = np.full((B, O), -1, np.int32), np.zeros((B, O), np.uint8)
        for b, n in enumerate(sizes):
            other[b, :n - 1], flip[b, :n - 1] = pair_draws(row["pairs"], n - 1, row["seed"] + b)
        out.update(other=other, flip=flip)
    if row["vocab"] == "clevr":
        import clevr_graph_cases as gc
        rels = []
        for b, n in enumerate(sizes):                  # every key a total order of the family's rank, seeded per key
            m = n - 1
            rank = {"chain": np.arange(m), "reverse_chain": np.arange(m)[::-1]}.get(row["family"])
            sc = {}
            for k, key in enumerate(gc.KEYS):
                perm = np.random.default_rng(row["seed"] + 10 * b + k).permutation(m) if rank is None else np.roll(rank, k)
                sc[key] = gc.order_rel([int(v) for v in perm])
            rels.append(np.asarray([[o2, gc.PREDS[key], o1] for key in sc for o1 in range(m) for o2 in sc[key][o1]],
                                   np.int64).reshape(-1, 3))
        R = max([len(r) for r in rels] + [1])
        rel = np.zeros((B, R, 3), np.int64)
        rel[:, :, 1] = gc.PREDS["__padding__"]
        for b, r in enumerate(rels):
            rel[b, :len(r)] = r
        out["rel"] = rel
    if row["conv"]:
        rng = np.random.default_rng(100 + row["seed"])
        P = len(p2i)
        w = rng.normal(size=(P, P)).astype(f32)
        out["weights"] = np.triu(w) + np.triu(w).T
        out["uniforms"] = rng.random(60000)
    return out


class Stream:
    """The uniform numbers as an iterator that counts what was taken."""

    def __init__(self, u):
        self.u, self.taken = u, 0

    def __iter__(self):
        return self

    def __next__(self):
        self.taken += 1
        return self.u[self.taken - 1]


_EXPECTED = {}


def expected(row):
    """The restatement's answer for a row, computed once and shared (read-only): triplets (B,T,3), tt (B,T), counts (B,),
    conv (B,P,P+1) float32, draws = the uniform numbers consumed."""
    if row["id"] in _EXPECTED:
        return _EXPECTED[row["id"]]
    assert not row["refused"]
    a = inputs(row)
    vocab, n = a["vocab"], a["n"]
    trans, dummies, conv = bool(row["trans"]), bool(row["dummies"]), bool(row["conv"])
    P = len(vocab["pred_name_to_idx"])
    pad = vocab["pred_name_to_idx"]["__padding__"]
    stream = Stream(a["uniforms"]) if conv else None
    w = a.get("weights")
    cc = None
    if row["vocab"] == "clevr":
        import clevr_graph_cases as gc
        trip, counts = gc.batch(a["rel"], n, int(trans))
        tt = np.zeros(trip.shape[:2], np.int64)
    elif row["pairs"]:
        import pair_cases as pc
        assert dummies
        rows = [pc.pair_rows_atan2(a["boxes"][b], a["centers"][b], int(n[b]) - 1, a["other"][b], a["flip"][b],
                                   vocab["pred_name_to_idx"], bool(row["use_converse"])) for b in range(len(n))]
        trip, tt, cc = pc.batch_from_rows(pc.padded_rows(rows, a["objs"].shape[1], vocab["pred_name_to_idx"]), n - 1, vocab,
                                          learned_transitivity=trans, learned_converse=conv, converse_weights=w, uniforms=stream)
        counts = (trip[:, :, 1] != pad).sum(1)
    elif "general_rows" in row["paths"] or "small" in row["paths"]:
        import vg_unpacked_cases as vu
        trip, tt, counts, cc = vu.annotated_batch(a["objs"], n, a["rel"], vocab, trans, dummies, conv, w, stream)
    elif row["annotated"] or P != 8:
        import canon_annotated as ca
        rel = a["rel"] if row["annotated"] else np.zeros((len(n), 0, 3), np.int64)
        trip, tt, counts, cc = ca.canonical_batch(a["objs"], a["boxes"], a["centers"], n, rel, vocab, trans, dummies, conv, w, stream)
    else:
        from oracle import canon
        r = canon.canonical_batch(a["objs"], a["boxes"], a["centers"], n, vocab, trans, dummies, conv, w, stream)
        trip, tt, counts = r[:3]
        cc = r[3] if conv else None
    cc = np.zeros((len(n), P, P + 1), f32) if cc is None or not conv else np.asarray(cc, f32)
    out = {"triplets": trip, "tt": tt, "counts": np.asarray(counts, np.int64), "conv": cc, "draws": stream.taken if conv else 0}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _EXPECTED[row["id"]] = out
    return out
