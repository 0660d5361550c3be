"""The cases of KID and the object-level FID (csrc/quality.hip, canonicalsg2im_amd/quality.py) and restatements of their rules in
numpy / torch, written from include/csg_hip.h and independent of the package: nothing here imports it.

  windows      `windows_ref`: the fp32 window rule, one numpy float32 operation per device operation
  crops        `cut`: the window cut out on the host; `interpolate64`: F.interpolate in fp64 on it
  KID          `kid_sums_ref`: the three kernel sums (and the sums of |k| the tolerance is built from) in fp64,
               `mmd2`, `draw_subsets`: the subsets as quality.kid_from_features draws them
  class sums   `class_sums_ref`
"""
import numpy as np
import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------ windows
H, W = 9, 13
NAN, INF = float("nan"), float("inf")

# (name, [x, y, w, h], [X0, Y0, X1, Y1) worked by hand from the rule).  fl(k / 13) * 13 and fl(k / 9) * 9 are exactly k in
# fp32 for every k used as a border below (k = 7 of 13 is the one that is not: 7.0000005, the row "fp32 decides").
WINDOW_ROWS = [
    ("whole picture", [0.0, 0.0, 1.0, 1.0], [0, 0, 13, 9]),
    ("one pixel", [0.0, 0.0, 1 / 13, 1 / 9], [0, 0, 1, 1]),
    ("edges on pixel borders", [2 / 13, 1 / 9, 3 / 13, 4 / 9], [2, 1, 5, 5]),
    # 0.2 * 13 = 2.6 -> 2, 0.5 * 13 = 6.5 -> 7; 0.3 * 9 = 2.7 -> 2, 0.65 * 9 = 5.85 -> 6
    ("edges between pixel borders", [0.2, 0.3, 0.3, 0.35], [2, 2, 7, 6]),
    # x = 4/13 on a border and w = 0: floor 4, ceil 4 -> X1 = X0 + 1; 0.5 * 9 = 4.5 -> 4, 0.75 * 9 = 6.75 -> 7
    ("zero width", [4 / 13, 0.5, 0.0, 0.25], [4, 4, 5, 7]),
    # 0.5 * 13 = 6.5 -> 6, 0.75 * 13 = 9.75 -> 10; y = 3/9 on a border and h = 0 -> Y1 = Y0 + 1
    ("zero height", [0.5, 3 / 9, 0.25, 0.0], [6, 3, 10, 4]),
    ("overhanging every edge", [-0.25, -0.25, 1.5, 1.5], [0, 0, 13, 9]),
    # -1.3 -> floor -2 -> 0, 0.2 * 13 = 2.6 -> 3; 0.2 * 9 = 1.8 -> 1, 0.4 * 9 = 3.6 -> 4
    ("x < 0", [-0.1, 0.2, 0.3, 0.2], [0, 1, 3, 4]),
    # 10.4 -> 10, 1.3 * 13 = 16.9 -> 13; 6.3 -> 6, 1.3 * 9 = 11.7 -> 9
    ("x + w > 1", [0.8, 0.7, 0.5, 0.6], [10, 6, 13, 9]),
    ("entirely outside, right and below", [1.5, 1.5, 0.2, 0.2], [12, 8, 13, 9]),
    ("entirely outside, left and above", [-0.5, -0.5, 0.2, 0.2], [0, 0, 1, 1]),
    ("last column", [12 / 13, 0.0, 1 / 13, 1.0], [12, 0, 13, 9]),
    ("last row", [0.0, 8 / 9, 1.0, 1 / 9], [0, 8, 13, 9]),
    ("fp32 decides", [0.0, 0.0, 7 / 13, 1.0], [0, 0, 8, 9]),
    # ---- windows only: the rows below are never passed to the resample
    ("NaN", [NAN, NAN, NAN, NAN], [0, 0, 1, 1]),
    ("+inf", [INF, INF, INF, INF], [12, 8, 13, 9]),
    ("-inf", [-INF, -INF, -INF, -INF], [0, 0, 1, 1]),
    ("1e30", [1e30, 1e30, 1e30, 1e30], [12, 8, 13, 9]),
    # x + w = inf -> 13; y = NaN -> 0, y + h = NaN -> 0 -> Y0 + 1
    ("mixed", [0.5, NAN, INF, 0.1], [6, 0, 13, 1]),
]
N_FINITE = 14
BOXES = np.array([r[1] for r in WINDOW_ROWS], dtype=np.float32)
HAND_WINDOWS = np.array([r[2] for r in WINDOW_ROWS], dtype=np.int32)


def _guarded(v, side):
    """A value that is not >= 0 becomes 0, a value above the side becomes the side, before the cast."""
    out = np.zeros(v.shape, np.int32)
    ok = v >= np.float32(0)                                  # False for NaN
    big = ok & (v > np.float32(side))
    mid = ok & ~big
    out[big] = side
    out[mid] = v[mid].astype(np.int32)
    return out


def windows_ref(boxes, h, w):
    """(N,4) float32 [x, y, w, h] -> (N,4) int32 [X0, Y0, X1, Y1): every step one float32 operation."""
    b = np.asarray(boxes, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fx0, fx1 = b[:, 0] * np.float32(w), (b[:, 0] + b[:, 2]) * np.float32(w)
        fy0, fy1 = b[:, 1] * np.float32(h), (b[:, 1] + b[:, 3]) * np.float32(h)
        x0 = np.minimum(_guarded(np.floor(fx0), w), w - 1)
        y0 = np.minimum(_guarded(np.floor(fy0), h), h - 1)
        x1 = np.maximum(_guarded(np.ceil(fx1), w), x0 + 1)
        y1 = np.maximum(_guarded(np.ceil(fy1), h), y0 + 1)
    return np.stack([x0, y0, x1, y1], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ crops
CROP_SIZES = [(5, 7), (9, 13), (4, 4)]                     # every finite row; (299, 299) for CROP_ROWS_299 only
CROP_ROWS_299 = [3, 8]
AFFINES = [(1.0, 0.0, False), (2.0, -1.0, False), (2.0, -1.0, True)]
IMAGE_INDEX = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1], dtype=np.int32)


def crop_pictures():
    """Two 9 x 13 pictures of random bytes, uint8 (2,9,13,3)."""
    return np.random.RandomState(7).randint(0, 256, (2, H, W, 3)).astype(np.uint8)


def cut(pictures, window, index):
    x0, y0, x1, y1 = (int(v) for v in window)
    return np.ascontiguousarray(pictures[int(index), y0:y1, x0:x1])


def interpolate64(window_u8, size, a, b, reverse):
    """F.interpolate(bilinear, align_corners=False) of the cut window in fp64, then a * v + b: (3,OH,OW) float64."""
    x = torch.from_numpy(window_u8.astype(np.float64) / 255.0).permute(2, 0, 1)[None]
    if reverse:
        x = x.flip(1)
    return (F.interpolate(x, size=size, mode="bilinear", align_corners=False) * a + b)[0]


# ------------------------------------------------------------------------------------------------ KID
# (nx, ny, m, D, S): m = 2; one tile with a tail; exactly one tile; a tile plus one row; three tiles, diagonal and off-diagonal
KID_CASES = [(5, 4, 2, 64, 1), (70, 90, 63, 64, 3), (64, 64, 64, 64, 2), (200, 150, 65, 192, 3), (300, 260, 130, 192, 2)]
KID_SEED = 0


def kid_features(nx, ny, D, signed=False):
    x = np.random.RandomState(1).randn(nx, D)
    y = np.random.RandomState(2).randn(ny, D) + (0.0 if signed else 0.3)
    if not signed:
        x, y = np.abs(x), np.abs(y)
    return x.astype(np.float32), y.astype(np.float32)


def draw_subsets(n0, n1, m, S, seed=KID_SEED):
    rng = np.random.RandomState(seed)
    ix, iy = np.empty((S, m), np.int32), np.empty((S, m), np.int32)
    for s in range(S):
        ix[s] = rng.choice(n0, m, replace=False)
        iy[s] = rng.choice(n1, m, replace=False)
    return ix, iy


def kid_sums_ref(fx, fy, ix, iy, gamma, coef0, degree):
    """-> (sums (S,3), sums of |k| over the same entries (S,3)) in float64."""
    S, m = ix.shape
    off = ~np.eye(m, dtype=bool)
    sums, mags = np.zeros((S, 3)), np.zeros((S, 3))
    for s in range(S):
        X, Y = fx[ix[s]].astype(np.float64), fy[iy[s]].astype(np.float64)
        for k, (A, B, mask) in enumerate(((X, X, off), (Y, Y, off), (X, Y, np.ones((m, m), bool)))):
            K = (gamma * (A @ B.T) + coef0) ** degree
            sums[s, k], mags[s, k] = K[mask].sum(), np.abs(K[mask]).sum()
    return sums, mags


def mmd2(sums, m):
    sums = np.asarray(sums, np.float64)
    return sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)


def kid_tolerances(mags, m, D):
    """Per sum 16 (3 D + m^2) 2^-53 sum |k| — the worst-case rounding of the dot product and the power (3 D eps) and of the
    m^2 additions, times 16 — and the same propagated through MMD^2."""
    tol = 16 * (3 * D + m * m) * 2.0 ** -53 * np.asarray(mags, np.float64)
    return tol, tol[:, 0] / (m * (m - 1)) + tol[:, 1] / (m * (m - 1)) + 2 * tol[:, 2] / (m * m)


# ------------------------------------------------------------------------------------------------ class sums
CLASS_N, CLASS_D, CLASS_C = 37, 64, 5


def class_case():
    """Two updates of (features (37,64) float32, ids (37) int32): class 3 is empty, one id is -1 and one is C."""
    rng = np.random.RandomState(11)
    parts = []
    for _ in range(2):
        ids = rng.choice([0, 1, 2, 4], CLASS_N).astype(np.int32)
        ids[5], ids[20] = -1, CLASS_C
        parts.append((rng.randn(CLASS_N, CLASS_D).astype(np.float32), ids))
    return parts


def class_sums_ref(parts, C):
    D = parts[0][0].shape[1]
    sums, mags, counts = np.zeros((C, D)), np.zeros((C, D)), np.zeros(C, np.int64)
    for x, ids in parts:
        for c in range(C):
            rows = x[ids == c].astype(np.float64)
            sums[c] += rows.sum(0)
            mags[c] += np.abs(rows).sum(0)
            counts[c] += rows.shape[0]
    return sums, mags, counts


# ------------------------------------------------------------------------------------------------ layouts
def layouts_doc():
    """A small layouts.json: string and dict names, a non-finite box, a small box; image 9 has no predicted boxes' twin."""
    return {"split": "val", "images": [
        {"image_id": 3, "objects": ["cube", {"shape": "sphere", "color": "red"}, "cube"],
         "gt_boxes": [[0.1, 0.1, 0.5, 0.5], [0.2, 0.3, 0.1, 0.1], [0.0, 0.0, NAN, 0.2]],
         "predicted_boxes": [[0.15, 0.1, 0.5, 0.4], [0.2, 0.3, 0.2, 0.2], [0.0, 0.0, 0.3, 0.2]]},
        {"image_id": "a7", "objects": [{"color": "red", "shape": "sphere"}, "cylinder"],
         "gt_boxes": [[0.5, 0.5, 0.4, 0.4], [0.0, 0.6, 0.05, 0.1]],
         "predicted_boxes": [[0.5, 0.5, 0.3, 0.4], [0.0, 0.6, 0.5, 0.1]]},
    ]}


def pictures(n, side, seed):
    """uint8 (n, side, side, 3): smooth blobs plus noise, so that crops of different places differ."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64) / side
    out = np.empty((n, side, side, 3), np.uint8)
    for i in range(n):
        for c in range(3):
            fx, fy, ph = rng.uniform(1, 4, 3)
            v = 0.5 + 0.35 * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph) + 0.1 * rng.randn(side, side)
            out[i, :, :, c] = np.clip(v * 255, 0, 255).astype(np.uint8)
    return out
