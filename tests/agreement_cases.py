"""Relation agreement (csg_relation_agreement, ops.relation_agreement): a numpy restatement of the entry's contract and the
table of cases the device is held to.

`restate` follows include/csg_hip.h word for word, in fp32 numpy: clamp the boxes to [0,1] as xywh (a NaN stays NaN),
xc = x0 + 0.5f * w as one fp32 addition, the centre from `centers` or (xc, yc), then the pair rule of
sg2im/data/base_dataset.py:42-81 per triplet.  Everything it returns is an integer: the comparisons with the device are
exact, and tests/test_agreement_cases.py holds the restatement itself to the reference's own verdicts
(tests/golden/clevr_syn.npz, part c).

The table: B in {1, 3}; T in {1, 63, 64, 65, 257} — below, at and past one wave, and past one block of 256 rows; O in
{2, 31}; both with and without `centers`; two vocabularies (the packed one, ids 0..7, and one of ten predicates whose
location ids are scattered).  Boxes lie on a grid of 1/16, so exact ties in x0, in the centre and in both occur; every
sample holds a box outside [0,1], a box with a NaN, and a pair nested both ways (with O = 2 the samples take turns)."""
import itertools

import numpy as np

NAMES = ("__padding__", "__in_image__", "__below__", "__above__", "__left of__", "__right of__", "__inside__", "__surrounding__")
PACKED = {n: i for i, n in enumerate(NAMES)}
SCATTERED = {"__padding__": 0, "riding": 1, "__in_image__": 2, "__surrounding__": 3, "__left of__": 4, "__below__": 5,
             "wearing": 6, "__inside__": 7, "__above__": 8, "__right of__": 9}


def vocab_of(table):
    names = sorted(table, key=table.get)
    return {"pred_name_to_idx": dict(table), "pred_idx_to_name": names}


def clamp01(x):
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1))         # numpy's min / max keep a NaN, as torch.clamp


def restate(boxes, centers, triplets, triplet_type, table):
    """-> tested (B,T) uint8, agrees (B,T) uint8, per_sample (B,4,2) int64, totals (4,P,2) int64 of this one call."""
    boxes = clamp01(np.asarray(boxes, np.float32))
    B, O = boxes.shape[:2]
    T, P = triplets.shape[1], len(table)
    x0, y0 = boxes[..., 0], boxes[..., 1]
    xc = x0 + np.float32(0.5) * boxes[..., 2]
    yc = y0 + np.float32(0.5) * boxes[..., 3]
    assert xc.dtype == np.float32
    cx, cy = (xc, yc) if centers is None else (np.asarray(centers, np.float32)[..., 0], np.asarray(centers, np.float32)[..., 1])
    s, p, o = (np.asarray(triplets[..., k], np.int64) for k in range(3))
    ty = np.asarray(triplet_type, np.int64)
    location = np.isin(p, [table[n] for n in NAMES[2:]])
    tested = location & (s >= 0) & (s < O) & (o >= 0) & (o < O) & (ty >= 0) & (ty < 4)
    ss, oo = np.where(tested, s, 0), np.where(tested, o, 0)
    take = lambda a, i: np.take_along_axis(a, i, 1)
    sx0, sy0, sxc, syc, scx, scy = (take(a, ss) for a in (x0, y0, xc, yc, cx, cy))
    ox0, oy0, oxc, oyc, ocx, ocy = (take(a, oo) for a in (x0, y0, xc, yc, cx, cy))
    nan = np.zeros((B, T), bool)
    for a in (sxc, syc, oxc, oyc, scx, scy, ocx, ocy):
        nan |= np.isnan(a)
    with np.errstate(invalid="ignore"):
        sur = (sx0 < ox0) & (sxc > oxc) & (sy0 < oy0) & (syc > oyc)
        ins = (sx0 > ox0) & (sxc < oxc) & (sy0 > oy0) & (syc < oyc)
        plain = ~sur & ~ins
        holds = {"__surrounding__": sur, "__inside__": ~sur & ins, "__right of__": plain & (scx > ocx),
                 "__left of__": plain & (scx < ocx), "__below__": plain & (scy > ocy), "__above__": plain & (scy < ocy)}
    agrees = np.zeros((B, T), bool)
    for name, h in holds.items():
        agrees |= (p == table[name]) & h
    agrees &= tested & ~nan
    per_sample = np.zeros((B, 4, 2), np.int64)
    totals = np.zeros((4, P, 2), np.int64)
    for b, t in zip(*np.nonzero(tested)):
        per_sample[b, ty[b, t]] += (int(agrees[b, t]), 1)
        totals[ty[b, t], p[b, t]] += (int(agrees[b, t]), 1)
    return tested.astype(np.uint8), agrees.astype(np.uint8), per_sample, totals


CASES = [(B, T, O, own, k % 2) for k, (B, T, O, own) in enumerate(itertools.product((1, 3), (1, 63, 64, 65, 257), (2, 31),
                                                                                   (False, True)))]


def case_id(case):
    return "B%d-T%d-O%d-%s-%s" % (case[0], case[1], case[2], "centers" if case[3] else "boxcentres",
                                  "scattered" if case[4] else "packed")


def make_case(case):
    """-> (boxes (B,O,4) f32, centers (B,O,2) f32 or None, triplets (B,T,3) i64, triplet_type (B,T) i64, table)."""
    B, T, O, own, scattered = case
    table = SCATTERED if scattered else PACKED
    rng = np.random.default_rng(1000 * B + 10 * T + O + 7 * own)
    boxes = np.concatenate([rng.integers(0, 9, (B, O, 2)), rng.integers(1, 8, (B, O, 2))], -1).astype(np.float32) / 16
    nan = np.float32("nan")
    for b in range(B):
        special = [np.asarray([-0.25, 0.5, 1.5, 0.25], np.float32),            # outside [0,1]: clamps to (0, .5, 1, .25)
                   np.asarray([0.25, 0.25, nan, 0.25], np.float32),            # a NaN width
                   np.asarray([0.125, 0.125, 0.75, 0.75], np.float32),         # surrounds the next
                   np.asarray([0.25, 0.25, 0.25, 0.25], np.float32)]
        if O >= 8:
            boxes[b, :4] = special
            boxes[b, 5] = boxes[b, 4]                                           # a tie in x0, y0 and both centres
            boxes[b, 6, 0], boxes[b, 6, 2] = boxes[b, 4, 0], boxes[b, 4, 2]     # a tie in x0 and the x centre alone
            boxes[b, 7, :2] = boxes[b, 4, :2]
            boxes[b, 7, 2:] = boxes[b, 4, 2:] + np.float32(0.125)               # a tie in x0, y0, not in the centre
        else:                                                                  # two objects: the samples and T take turns
            kind = (b + T) % 4
            boxes[b, 0], boxes[b, 1] = (special[2], special[3]) if kind == 0 else (special[3], special[3]) if kind == 1 else \
                (special[1], special[3]) if kind == 2 else (special[0], special[3])
    centers = None
    if own:                                        # centres of their own, on the grid too: ties with and against the boxes'
        centers = (rng.integers(0, 5, (B, O, 2)).astype(np.float32) / 4)
        if O >= 8:
            centers[:, 9, 0] = nan                 # a NaN centre under a clean box
    ids = np.asarray(sorted(table.values()), np.int64)
    triplets = np.stack([rng.integers(0, O, (B, T)), ids[rng.integers(0, len(ids), (B, T))], rng.integers(0, O, (B, T))], -1)
    triplet_type = rng.integers(0, 4, (B, T)).astype(np.int64)
    if T >= 63:                                    # every predicate and every type, the nested pair asked both ways
        for k, name in enumerate(NAMES[2:]):
            triplets[:, 2 * k] = (2, table[name], 3) if O >= 8 else (0, table[name], 1)
            triplets[:, 2 * k + 1] = (3, table[name], 2) if O >= 8 else (1, table[name], 0)
        triplets[:, 12] = (0, table["__padding__"], 0)
        triplets[:, 13] = (0, table["__in_image__"], O - 1)
        triplet_type[:, :4] = np.arange(4)
    return boxes, centers, triplets.astype(np.int64), triplet_type, table
