"""Graph rewriting and layout consistency (csrc/rewrite.hip, csrc/csg_rewrite.h, csg_layout_consistency in
csrc/metrics.hip): numpy restatements of the entries' contracts and the tables of cases the device is held to
(tests/test_gpu_rewrite.py); tests/test_rewrite_cases.py holds the restatements themselves to fixed vectors and to the
golden scenes.

The hash is restated twice: `hash_py` in Python's unbounded integers (masked to 64 bits), from which HASH_VECTORS were
written down, and `hash_np` in numpy uint64, which the row rules use.  Integers only: every comparison with the device is
exact.  `restate_consistency` follows include/csg_hip.h word for word in fp32 numpy, including the association of the fp64
sums (thread o holds object o; a shuffle tree per 64; waves in order; samples in ascending order)."""
import itertools

import numpy as np

import agreement_cases as ac

NAMES = ac.NAMES
SLOTS = NAMES[2:]                                   # below 0, above 1, left of 2, right of 3, inside 4, surrounding 5
FORWARD_SLOTS = (1, 2, 4)                           # above, left of, inside
MODES = {"one_sided": 0, "noise": 1}
DIRECTIONS = {"forward": 0, "backward": 1, "random": 2}
M64 = (1 << 64) - 1
GAMMA = 0x9e3779b97f4a7c15


# ---- the hash, in Python integers -----------------------------------------------------------------------------------------
def fin_py(z):
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def step_py(h, w):
    return fin_py(((h ^ (w & M64)) + GAMMA) & M64)


def hash_py(seed, image, a, b, slot):
    h = step_py(0, seed)
    h = step_py(h, image)
    h = step_py(h, (a << 32) | b)
    return step_py(h, slot)


def threshold(share):
    return int(np.floor(np.float64(share) * 4294967296.0 + 0.5))


# (seed, image id, a, b, slot) -> h, and g = step(h, 1): written down from hash_py and from csrc/csg_rewrite.h compiled for
# the host; test_rewrite_cases.py holds both restatements to them
HASH_VECTORS = [
    (0x0, 0, 0, 0, 0, 0x2130748aaac80268, 0xa5d3758b95b92366),
    (0x0, 0, 0, 1, 2, 0x1a69f2b59aba5775, 0x8dbbad9f4c68c3c9),
    (0x0, 0, 1, 0, 2, 0x5a5cba748097e850, 0x527e34c6f96f9fb6),
    (0x1, 0, 0, 1, 2, 0xe4cc646401ae52aa, 0x4f81d16ae78f1518),
    (0x0, 1, 0, 1, 2, 0xc1ae2036d5caa152, 0xa9d7a950f9ef3982),
    (0x0, 7, 3, 5, 1, 0x9a60efc3952b101f, 0xbb8d866139679e47),
    (0x3039, 999983, 254, 17, 4, 0x8b4616f2d44d31cb, 0x7a850e8a60ec4634),
    (0xffffffffffffffff, -1, 2147483647, 2147483647, 5, 0x5f03152d73788706, 0xdb820e1616006ff9),
    (0x2a, 1000003, 11, 0, 3, 0x7b8135cfd57f2150, 0x7d78460496b143fb),
]


# ---- the hash, in numpy uint64 -------------------------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x).astype(np.uint64)              # an int64 image id wraps, as the kernel's cast does


def fin_np(z):
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xbf58476d1ce4e5b9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))


def step_np(h, w):
    with np.errstate(over="ignore"):
        return fin_np((h ^ w) + np.uint64(GAMMA))


def hash_np(seed, image, a, b, slot):
    h = step_np(np.uint64(0), np.uint64(seed))
    h = step_np(h, _u64(image))
    h = step_np(h, (_u64(a) << np.uint64(32)) | _u64(b))
    return step_np(h, _u64(slot))


# ---- the two entries of rewrite.hip ----------------------------------------------------------------------------------------
def restate_select(triplets, triplet_type, table, O):
    """-> rows (B,T,3) int64, counts (B,) int64"""
    triplets, triplet_type = np.asarray(triplets, np.int64), np.asarray(triplet_type, np.int64)
    B, T = triplet_type.shape
    rows = np.zeros((B, T, 3), np.int64)
    rows[..., 1] = table["__padding__"]
    counts = np.zeros(B, np.int64)
    location = [table[n] for n in SLOTS]
    for b in range(B):
        s, p, o = triplets[b, :, 0], triplets[b, :, 1], triplets[b, :, 2]
        wanted = np.isin(p, location) & (triplet_type[b] == 0)
        inside = (s >= 0) & (s < O) & (o >= 0) & (o < O)
        keep = triplets[b][wanted & inside]
        rows[b, :len(keep)] = keep
        counts[b] = -1 - len(keep) if (wanted & ~inside).any() else len(keep)
    return rows, counts


def restate_rewrite(rows, counts, image_ids, table, mode, share, direction="random", seed=0):
    """-> rows (B,R,3) int64: the first counts[b] rows of each sample rewritten"""
    rows = np.array(rows, np.int64)
    B, R = rows.shape[:2]
    thr = np.uint64(threshold(share))
    pid = np.asarray([table[n] for n in SLOTS], np.int64)
    slot = np.full((B, R), -1, np.int64)
    for k in range(6):
        slot[rows[..., 1] == pid[k]] = k
    s, o = rows[..., 0], rows[..., 2]
    live = (np.arange(R)[None] < np.asarray(counts, np.int64)[:, None]) & (slot >= 0) & (s >= 0) & (s < 2 ** 31) & (o >= 0) \
        & (o < 2 ** 31)
    image = np.broadcast_to(np.asarray(image_ids, np.int64)[:, None], (B, R))
    ks = np.where(live, slot, 0)
    if MODES[mode] == 0:
        fwd = np.isin(ks, FORWARD_SLOTS)
        a, b, kf = np.where(fwd, s, o), np.where(fwd, o, s), np.where(fwd, ks, ks ^ 1)
        h = hash_np(seed, image, np.where(live, a, 0), np.where(live, b, 0), kf)
        hit = live & ((h >> np.uint64(32)) < thr)
        coin = (step_np(h, np.uint64(1)) >> np.uint64(63)) == 0
        want_fwd = {0: np.ones((B, R), bool), 1: np.zeros((B, R), bool), 2: coin}[DIRECTIONS[direction]]
        new_s, new_o, new_k = np.where(want_fwd, a, b), np.where(want_fwd, b, a), np.where(want_fwd, kf, kf ^ 1)
    else:
        assert direction in DIRECTIONS
        h = hash_np(seed, image, np.where(live, s, 0), np.where(live, o, 0), ks)
        hit = live & ((h >> np.uint64(32)) < thr)
        r = (((step_np(h, np.uint64(1)) >> np.uint64(32)) * np.uint64(5)) >> np.uint64(32)).astype(np.int64)
        new_s, new_o, new_k = s, o, np.where(r < ks, r, r + 1)
    out = rows.copy()
    out[..., 0] = np.where(hit, new_s, s)
    out[..., 2] = np.where(hit, new_o, o)
    out[..., 1] = np.where(hit, pid[new_k], rows[..., 1])
    return out


def mirror_closure(rows, table):
    """The rows and every row's mirror (o, converse, s), np.unique: what two equivalent sets of rows have in common."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    pid = np.asarray([table[n] for n in SLOTS], np.int64)
    slot = np.asarray([int(np.nonzero(pid == p)[0][0]) for p in rows[:, 1]], np.int64).reshape(-1)
    mirrored = np.stack([rows[:, 2], pid[slot ^ 1] if len(rows) else rows[:, 1], rows[:, 0]], 1)
    return np.unique(np.concatenate([rows, mirrored]), axis=0)


# ---- select + rewrite cases ------------------------------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 63, 64, 65, 257)
SELECT_CASES = [(B, n, k % 2) for k, (B, n) in enumerate(itertools.product((1, 3), ROW_COUNTS))]
REWRITES = [("one_sided", share, d) for share in (0.0, 0.5, 1.0) for d in ("forward", "backward", "random")] + \
           [("noise", share, "random") for share in (0.0, 0.5, 1.0)]


def select_case_id(case):
    return "B%d-rows%d-%s" % (case[0], case[1], "scattered" if case[2] else "packed")


def make_select_case(case):
    """-> (triplets (B,T,3) i64, triplet_type (B,T) i64, image_ids (B,) i64, table, O).  Sample 0 holds exactly `n` rows
    to select, the others n + b; between them rows of __in_image__, TRANSITIVE (and other non-ORIGINAL) location rows
    and __padding__ rows, which must not be selected; the last sample of a B = 3 case holds one ORIGINAL location row
    whose object lies outside [0, O): its count is negative."""
    B, n, scattered = case
    table = ac.SCATTERED if scattered else ac.PACKED
    O = 12
    rng = np.random.default_rng(77 * B + n)
    pid = np.asarray([table[x] for x in SLOTS], np.int64)
    samples = []
    for b in range(B):
        rows = []
        for _ in range(n + b if n else 0):
            s, o = rng.choice(O, 2, replace=False)
            rows.append((s, pid[rng.integers(6)], o, 0))
            kind = rng.integers(4)
            if kind == 0:
                rows.append((rng.integers(O), table["__in_image__"], O - 1, 0))
            elif kind == 1:
                rows.append((rng.integers(O), pid[rng.integers(6)], rng.integers(O), 1 + rng.integers(3)))
            elif kind == 2:
                rows.append((0, table["__padding__"], 0, 0))
        if not rows:
            rows = [(1, table["__in_image__"], O - 1, 0), (2, pid[0], 3, 1)]
        if B == 3 and b == 2:
            rows.insert(len(rows) // 2, (3, pid[2], O, 0))
        samples.append(rows)
    T = max(len(r) for r in samples)
    triplets = np.zeros((B, T, 3), np.int64)
    triplets[..., 1] = table["__padding__"]
    ttype = np.zeros((B, T), np.int64)
    for b, rows in enumerate(samples):
        arr = np.asarray(rows, np.int64)
        triplets[b, :len(rows)], ttype[b, :len(rows)] = arr[:, :3], arr[:, 3]
    image_ids = np.asarray([1000003 * (n + 1) + 17 * b for b in range(B)], np.int64)
    return triplets, ttype, image_ids, table, O


# ---- layout consistency ------------------------------------------------------------------------------------------------------
def _clamp_box(b):
    return ac.clamp01(np.asarray(b, np.float32))


def _jaccard(p, g):
    """csg_box_iou's operations on two clamped boxes (N,4) fp32, each one fp32 operation in its order"""
    tmin = lambda a, b: np.where((a < b) | np.isnan(a), a, b)
    tmax = lambda a, b: np.where((a > b) | np.isnan(a), a, b)
    zero = np.float32(0)
    px0, py0, gx0, gy0 = p[:, 0], p[:, 1], g[:, 0], g[:, 1]
    px1, py1, gx1, gy1 = px0 + p[:, 2], py0 + p[:, 3], gx0 + g[:, 2], gy0 + g[:, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        ix = tmax(tmin(px1, gx1) - tmax(px0, gx0), zero)
        iy = tmax(tmin(py1, gy1) - tmax(py0, gy0), zero)
        inter = ix * iy
        area_p, area_g = (px1 - px0) * (py1 - py0), (gx1 - gx0) * (gy1 - gy0)
        out = inter / ((area_p + area_g) - inter)
    assert out.dtype == np.float32
    return out


def _verdicts(boxes):
    """boxes (O,4) fp32 -> bool (6, O, O): verdict [slot, i, j] of the pair rule for subject i, object j, box centres"""
    bx = _clamp_box(boxes)
    x0, y0 = bx[:, 0], bx[:, 1]
    xc, yc = x0 + np.float32(0.5) * bx[:, 2], y0 + np.float32(0.5) * bx[:, 3]
    nan = np.isnan(xc) | np.isnan(yc)
    S, Ob = (lambda a: a[:, None]), (lambda a: a[None, :])
    with np.errstate(invalid="ignore"):
        sur = (S(x0) < Ob(x0)) & (S(xc) > Ob(xc)) & (S(y0) < Ob(y0)) & (S(yc) > Ob(yc))
        ins = (S(x0) > Ob(x0)) & (S(xc) < Ob(xc)) & (S(y0) > Ob(y0)) & (S(yc) < Ob(yc))
        plain = ~sur & ~ins
        v = np.stack([plain & (S(yc) > Ob(yc)), plain & (S(yc) < Ob(yc)), plain & (S(xc) < Ob(xc)), plain & (S(xc) > Ob(xc)),
                      ~sur & ins, sur])
    return v & ~(S(nan) | Ob(nan))[None]


def _block_sum(v):
    """fp64 (256,) -> the block's ordered sum: a shuffle tree per wave of 64 (offsets 32 .. 1), then waves 1, 2, 3 in order"""
    w = np.array(v, np.float64).reshape(4, 64)
    with np.errstate(invalid="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            w[:, :off] = w[:, :off] + w[:, off:2 * off]
        total = w[0, 0]
        for k in (1, 2, 3):
            total = total + w[k, 0]
    return total


def restate_consistency(boxes_a, boxes_b, counted, totals_f, totals_i):
    """-> (iou_ab (B,O) f32, shift (B,O) f32, per_sample_f (B,4) f64, per_sample_i (B,20) i64, totals_f + , totals_i +)"""
    boxes_a, boxes_b = np.asarray(boxes_a, np.float32), np.asarray(boxes_b, np.float32)
    counted = np.asarray(counted).astype(bool)
    B, O = counted.shape
    iou = np.zeros((B, O), np.float32)
    shift = np.zeros((B, O), np.float32)
    per_f, per_i = np.zeros((B, 4), np.float64), np.zeros((B, 20), np.int64)
    for b in range(B):
        ca, cb = _clamp_box(boxes_a[b]), _clamp_box(boxes_b[b])
        half = np.float32(0.5)
        with np.errstate(invalid="ignore"):
            d = np.abs((ca[:, 0] + half * ca[:, 2]) - (cb[:, 0] + half * cb[:, 2])) + \
                np.abs((ca[:, 1] + half * ca[:, 3]) - (cb[:, 1] + half * cb[:, 3]))
            v = _jaccard(ca, cb)
            assert d.dtype == np.float32
            on = counted[b]
            iou[b], shift[b] = np.where(on, v, np.float32(0)), np.where(on, d, np.float32(0))
            lanes = np.zeros((4, 256), np.float64)
            lanes[0, :O] = np.where(on, v.astype(np.float64), 0.0)
            lanes[1, :O] = np.where(on & (v > np.float32(0.5)), 1.0, 0.0)
            lanes[2, :O] = np.where(on, d.astype(np.float64), 0.0)
            lanes[3, :O] = on
        per_f[b] = [_block_sum(lanes[q]) for q in range(4)]
        pair = on[:, None] & on[None, :] & ~np.eye(O, dtype=bool)
        va, vb = _verdicts(boxes_a[b]) & pair[None], _verdicts(boxes_b[b]) & pair[None]
        for k in range(6):
            per_i[b, 3 * k:3 * k + 3] = [va[k].sum(), vb[k].sum(), (va[k] & vb[k]).sum()]
        per_i[b, 18] = ((va == vb).all(0) & pair).sum()
        per_i[b, 19] = pair.sum()
    tf, ti = np.array(totals_f, np.float64), np.array(totals_i, np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(B):                              # ascending sample order, onto the running totals
            tf = tf + per_f[b]
            ti = ti + per_i[b]
    return iou, shift, per_f, per_i, tf, ti


CONSISTENCY_CASES = [(B, O, kind) for B in (1, 3) for O in (1, 2, 31, 64, 65, 255) for kind in ("moved", "identical")]


def consistency_case_id(case):
    return "B%d-O%d-%s" % case


def make_consistency_case(case):
    """-> (boxes_a, boxes_b (B,O,4) f32, counted (B,O) u8).  Boxes on a grid of 1/16 (exact ties occur) plus, in "moved",
    layout B moved off the grid; with O >= 8 every sample holds a box outside [0,1], a nested pair, an uncounted object
    and a tiny box (terms 2^-40 beside terms near 1: the fp64 sums round, so their association shows), and the first
    sample a zero-area box and, in some cases, a NaN box in B; the last sample of a B = 3 case has nothing counted."""
    B, O, kind = case
    rng = np.random.default_rng(31 * B + O + (5 if kind == "moved" else 0))
    a = np.concatenate([rng.integers(0, 9, (B, O, 2)), rng.integers(1, 8, (B, O, 2))], -1).astype(np.float32) / 16
    if O >= 8:
        a[:, 0] = (-0.25, 0.5, 1.5, 0.25)                                  # clamps to (0, .5, 1, .25)
        a[:, 2], a[:, 3] = (0.125, 0.125, 0.75, 0.75), (0.25, 0.25, 0.25, 0.25)      # 2 surrounds 3
        a[0, 4] = (0.5, 0.5, 0.0, 0.25)                                    # zero area: 0 / 0 against itself
        a[:, 7] = (1.1e-12, 2.3e-12, 3.7e-12, 0.9e-12)                     # tiny: its terms make the fp64 sums round
    b = a.copy()
    counted = np.ones((B, O), np.uint8)
    if kind == "moved":
        b[..., :2] += (rng.standard_normal((B, O, 2)) * 0.07).astype(np.float32)
        b[..., 2:] *= (1 + rng.standard_normal((B, O, 2)) * 0.1).astype(np.float32)
        if O >= 8:
            b[:, 7] = a[:, 7] * np.float32(1.37)
            if B == 3 or O == 31:                                          # elsewhere the sums stay finite
                b[0, 1, 2] = np.float32("nan")
            b[:, 5] = (1.25, -0.5, 0.5, 2.0)
            counted[:, 6] = 0
        elif O == 2 and B == 3:
            b[1, 0, 0] = np.float32("nan")
    if B == 3:
        counted[2] = 0
    return a, b, counted
