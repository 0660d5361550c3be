"""COCO segmentation masks: the reference's per-object recipe restated in integers and float64, and the table of cases
(tests/test_mask_cases.py pins the restatement on the CPU, tests/test_gpu_coco_masks.py holds csg_coco_masks and the two
COCO folder datasets to it).

What the reference does per object (sg2im/data/packed_coco.py:305-351, sg2im/data/coco.py:317-363): seg_to_mask through
pycocotools (frPyObjects / merge / decode), a crop to the rounded box, cv2.resize(..., (M, M), INTER_NEAREST), and the
centroid of the resized mask on torch.linspace(x0, x0 + w, M) as the object's centre.  Neither library is a dependency of
this package, so their algorithms are written out here, from their public sources:

  rle_from_poly      pycocotools' rleFrPoly (common/maskApi.c), scale 5: the toggles `a` of the column-major mask
  mask_from_toggles  value(i) = parity(#{a <= i}), i = x * HH + y
  column_crossings   the per-column shortcut the device uses: the crossings of ONE picture column, per edge in closed form
  rle_to_string / rle_from_string   pycocotools' rleToString / rleFrString
  seg_to_mask        the reference's dispatch: polygons (union), runs as a list, runs as a compressed string
  crop_of            int(round(.)) with ties to even, max(lo + 1, hi), then the clamp of a numpy slice
  resize_index       cv2's INTER_NEAREST source index: min(floor(c * ifx), cw - 1), ifx = 1.0 / ((double) M / cw)
  object_mask        the three in a row -> (M, M) int64
  centre_closed      the centre in fp64, rounded once to fp32 — the device's formula, bit for bit
  centre_torch       the reference's own fp32 recipe (torch.linspace, boolean index, mean)

Pictures of the table are 9 to 40 pixels on a side, with ONE exception: a run of at least 2^15 pixels — the count that takes
four characters in the compressed string — does not fit a 40 x 40 picture (1600 pixels), so the last picture of the second
batch is 200 x 180."""
import json
import math
import os

import numpy as np

f32 = np.float32
SCALE = 5.0
MASK_SIZES = (2, 4, 16, 32, 64)


# ------------------------------------------------------------------------------------------------ polygons: the flat rule
def _vertices(xy):
    xy = np.asarray(xy, np.float64).reshape(-1)
    k = xy.shape[0] // 2
    X = [int(SCALE * xy[2 * j] + .5) for j in range(k)]          # C's (int): truncation
    Y = [int(SCALE * xy[2 * j + 1] + .5) for j in range(k)]
    return X, Y


def boundary_points(xy):
    """The dense boundary of rleFrPoly -> (u, v) int64 arrays, edge after edge, every edge with both its ends."""
    X, Y = _vertices(xy)
    k = len(X)
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[(j + 1) % k], Y[j], Y[(j + 1) % k]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        n = max(dx, dy)
        d = np.arange(n + 1, dtype=np.int64)
        t = (n - d) if flip else d
        if n == 0:                                               # 0 / 0 in C: the slope is never used
            us.append(np.asarray([xs], np.int64))
            vs.append(np.asarray([ys], np.int64))
        elif dx >= dy:
            s = float(ye - ys) / dx
            us.append(t + xs)
            vs.append((ys + s * t.astype(np.float64) + .5).astype(np.int64))       # astype truncates, as (int) does
        else:
            s = float(xe - xs) / dy
            us.append((xs + s * t.astype(np.float64) + .5).astype(np.int64))
            vs.append(t + ys)
    if not us:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(us), np.concatenate(vs)


def rle_from_poly(xy, HH, WW):
    """rleFrPoly's toggles, unsorted: a = xd * HH + yd for every change of u that falls on a pixel column."""
    u, v = boundary_points(xy)
    a = []
    for j in range(1, u.shape[0]):
        if u[j] == u[j - 1]:
            continue
        xd = (float(min(u[j], u[j - 1])) + .5) / SCALE - .5
        if math.floor(xd) != xd or xd < 0 or xd > WW - 1:
            continue
        yd = (float(min(v[j], v[j - 1])) + .5) / SCALE - .5
        yd = math.ceil(min(max(yd, 0.0), float(HH)))
        a.append(int(xd) * HH + int(yd))
    return a


def mask_from_toggles(a, HH, WW):
    """value(i) = parity(#{a <= i}) over i = x * HH + y -> (HH, WW) uint8."""
    a = np.asarray(a, np.int64).reshape(-1)
    hits = np.bincount(a[(a >= 0) & (a < HH * WW)], minlength=HH * WW)
    return (np.cumsum(hits) & 1).astype(np.uint8).reshape(WW, HH).T.copy()


def poly_mask_flat(xy, HH, WW):
    return mask_from_toggles(rle_from_poly(xy, HH, WW), HH, WW)


# ------------------------------------------------------------------------------------------------ polygons: per column
def column_crossings(xy, X, HH):
    """The yd of every crossing of picture column X (an integer >= 0), one edge at a time and without the point list: the
    level lies between u = 5 X + 2 and 5 X + 3; an edge with dx >= dy meets it at t = U - xs, an edge with dx < dy where
    u(t) = (int)(xs + s t + .5), monotone in t, passes it — found by bisection.  yd as rle_from_poly gives it."""
    Xs, Ys = _vertices(xy)
    k = len(Xs)
    U = 5 * X + 2
    out = []
    for j in range(k):
        xs, xe, ys, ye = Xs[j], Xs[(j + 1) % k], Ys[j], Ys[(j + 1) % k]
        dx, dy = abs(xe - xs), abs(ys - ye)
        if (dx >= dy and xs > xe) or (dx < dy and ys > ye):
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            if not (xs <= U < xe):
                continue
            s = float(ye - ys) / dx
            t0 = U - xs
            mv = min(int(ys + s * t0 + .5), int(ys + s * (t0 + 1) + .5))
        else:
            s = float(xe - xs) / dy
            if s == 0:
                continue

            def passed(t):
                u = int(xs + s * t + .5)
                return u >= U + 1 if s > 0 else u <= U

            if passed(0) or not passed(dy):
                continue
            lo, hi = 0, dy                                       # passed(lo) is False, passed(hi) is True
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if passed(mid):
                    hi = mid
                else:
                    lo = mid
            mv = ys + hi - 1
        yd = (float(mv) + .5) / SCALE - .5
        out.append(int(math.ceil(min(max(yd, 0.0), float(HH)))))
    return out


def poly_mask_columns(xy, HH, WW):
    """The mask by the per-column rule: value(x, y) = parity(#{crossings of column x with yd <= y}) -> ((HH, WW) uint8,
    the largest number of crossings of a column modulo 2: 0 when every column has an even number)."""
    out = np.zeros((HH, WW), np.uint8)
    odd = 0
    for x in range(WW):
        yds = column_crossings(xy, x, HH)
        odd |= len(yds) & 1
        for yd in yds:
            out[yd:, x] ^= 1
    return out, odd


# ------------------------------------------------------------------------------------------------ runs
def runs_of(mask):
    """The column-major run lengths of a (HH, WW) 0/1 mask, starting with the zeros (pycocotools' rleEncode)."""
    flat = np.asarray(mask, np.uint8).T.reshape(-1)
    counts, prev, run = [], 0, 0
    for v in flat.tolist():
        if v != prev:
            counts.append(run)
            run, prev = 0, v
        run += 1
    counts.append(run)
    return counts


def rle_to_string(counts):
    """rleToString: the difference to the count two places back from the fourth count on, five bits per character plus a
    continuation bit, characters 48 .. 111."""
    out = []
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5                                              # arithmetic shift, as C's on a long
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return "".join(out)


def rle_from_string(s):
    """rleFrString, one character at a time -> the counts."""
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def toggles_of(counts):
    return np.cumsum(np.asarray(counts, np.int64))


# ------------------------------------------------------------------------------------------------ the object's recipe
def seg_to_mask(seg, WW, HH):
    """The reference's seg_to_mask -> (HH, WW) uint8."""
    if isinstance(seg, list):
        out = np.zeros((HH, WW), np.uint8)
        for poly in seg:
            out |= poly_mask_flat(poly, HH, WW)                  # merge: a union
        return out
    if list(seg["size"]) != [HH, WW]:
        raise ValueError("size %s is not the picture's %s" % (seg["size"], [HH, WW]))
    counts = seg["counts"] if isinstance(seg["counts"], list) else rle_from_string(seg["counts"])
    return mask_from_toggles(toggles_of(counts), HH, WW)


def crop_of(bbox, WW, HH):
    """(x0, y0, x1, y1) of mask[my0:my1, mx0:mx1]: Python's round, max(lo + 1, hi), the clamp of a slice."""
    x, y, w, h = bbox
    mx0, mx1 = int(round(x)), int(round(x + w))
    my0, my1 = int(round(y)), int(round(y + h))
    mx1, my1 = max(mx0 + 1, mx1), max(my0 + 1, my1)
    x0, x1, _ = slice(mx0, mx1).indices(WW)
    y0, y1, _ = slice(my0, my1).indices(HH)
    return x0, y0, max(x0, x1), max(y0, y1)


def resize_index(M, cw):
    """cv2.resize's INTER_NEAREST source index of the M destination positions over `cw` source positions."""
    ifx = 1.0 / (float(M) / cw)
    return np.asarray([min(int(math.floor(c * ifx)), cw - 1) for c in range(M)], np.int64)


def object_mask(seg, bbox, WW, HH, M):
    x0, y0, x1, y1 = crop_of(bbox, WW, HH)
    crop = seg_to_mask(seg, WW, HH)[y0:y1, x0:x1]
    if crop.size == 0:
        raise ValueError("empty crop")
    return crop[resize_index(M, y1 - y0)][:, resize_index(M, x1 - x0)].astype(np.int64)


def box_of(bbox, WW, HH):
    """The reference's fp32 box: Python floats divided, rounded once."""
    x, y, w, h = bbox
    return np.asarray([x / WW, y / HH, w / WW, h / HH], np.float64).astype(f32)


def centre_closed(box, mask):
    """(x, y) fp32 of an object with fp32 box (x0, y0, w, h) and (M, M) mask: the box centre in fp32 for an empty mask, else
    x0 + ((fp32)(x0 + w) - x0) * sum(col) / ((M - 1) * count) in fp64, rounded once."""
    box = np.asarray(box, f32)
    mask = np.asarray(mask)
    M = mask.shape[0]
    count = int(mask.sum())
    if count == 0:
        return np.asarray([box[0] + f32(0.5) * box[2], box[1] + f32(0.5) * box[3]], f32)
    rows, cols = np.nonzero(mask)
    out = []
    for lo, ext, tot in ((box[0], box[2], int(cols.sum())), (box[1], box[3], int(rows.sum()))):
        hi = f32(lo + ext)                                       # fp32, as the reference's tensor sum
        d = np.float64(hi) - np.float64(lo)
        out.append(f32(np.float64(lo) + (d * np.float64(tot)) / np.float64((M - 1) * count)))
    return np.asarray(out, f32)


def centre_torch(box, mask):
    """packed_coco.py:339-350 as written, on fp32 CPU tensors."""
    import torch
    x0, y0, w, h = torch.from_numpy(np.array(box, f32))
    m = torch.from_numpy(np.array(mask)) == 1
    MH, MW = m.shape
    xs = torch.linspace(x0, x0 + w, MW).view(1, MW).expand(MH, MW)
    ys = torch.linspace(y0, y0 + h, MH).view(MH, 1).expand(MH, MW)
    if m.sum() == 0:
        return np.asarray([float(x0 + 0.5 * w), float(y0 + 0.5 * h)], f32)
    return np.asarray([float(xs[m].mean()), float(ys[m].mean())], f32)


def ulps(a, b):
    """|a - b| in units of the last place of b (fp32)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the table
def _rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def _star(cx, cy, r):
    pts = []
    for i in range(5):
        ang = math.radians(-90 + 144 * i)
        pts += [round(cx + r * math.cos(ang), 2), round(cy + r * math.sin(ang), 2)]
    return pts


def _ellipse(HH, WW, cx, cy, rx, ry):
    yy, xx = np.mgrid[0:HH, 0:WW]
    return ((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1.0).astype(np.uint8)


def _big_runs():
    """200 x 180 (WW x HH): 33000 zeros — a count of at least 2^15 — then 500 ones, then zeros."""
    return [33000, 500, 200 * 180 - 33500]


def table():
    """[batch][sample] = {"size": (WW, HH), "objects": [{"what", "bbox", "segmentation"}]}: two batches of 3 samples with 1,
    3 and 5 objects.  One row per behaviour that can go wrong."""
    ell = _ellipse(180, 200, 60.0, 90.0, 30.0, 50.0)
    ell_counts = runs_of(ell)
    list_mask = _ellipse(180, 200, 120.5, 40.0, 25.0, 18.0)
    big = _big_runs()
    circle = []
    for i in range(24):
        circle += [round(100 + 40 * math.cos(2 * math.pi * i / 24), 2), round(120 + 35 * math.sin(2 * math.pi * i / 24), 2)]
    return [
        [
            {"size": (24, 20), "objects": [
                {"what": "triangle", "bbox": [3.0, 2.0, 17.0, 15.0], "segmentation": [[3, 2, 20, 5, 8, 17]]}]},
            {"size": (40, 32), "objects": [
                {"what": "concave L", "bbox": [2.0, 2.0, 28.0, 26.0],
                 "segmentation": [[2, 2, 30, 2, 30, 6, 6, 6, 6, 28, 2, 28]]},
                {"what": "second object of the L's pair", "bbox": [1.0, 1.0, 24.0, 22.0], "segmentation": [_rect(1, 1, 25, 23)]},
                {"what": "self-crossing star", "bbox": [22.0, 14.0, 16.0, 16.0], "segmentation": [_star(30, 22, 8)]}]},
            {"size": (33, 27), "objects": [
                {"what": "partly outside all four borders", "bbox": [0.0, 0.0, 33.0, 27.0],
                 "segmentation": [[16, -6, 40, 13, 16, 33, -7, 13]]},
                {"what": "repeated vertex", "bbox": [4.0, 4.0, 8.0, 8.0], "segmentation": [[4, 4, 12, 4, 12, 4, 12, 12, 4, 12]]},
                {"what": "half-integer and two-decimal coordinates", "bbox": [5.5, 6.5, 14.75, 13.0],
                 "segmentation": [[5.5, 6.5, 20.25, 7.75, 18.37, 19.5, 6.12, 17.88]]},
                {"what": "sliver that rasterises empty", "bbox": [10.0, 5.0, 1.0, 15.0],
                 "segmentation": [[10.0, 5.0, 10.1, 5.0, 10.1, 20.0]]},
                {"what": "two overlapping polygons", "bbox": [2.0, 2.0, 18.0, 18.0],
                 "segmentation": [_rect(2, 2, 14, 14), _rect(8, 8, 20, 20)]}]},
        ],
        [
            {"size": (9, 11), "objects": [
                {"what": "x = 2.5: round ties to even", "bbox": [2.5, 1.5, 4.0, 5.0], "segmentation": [_rect(2, 1, 7, 7)]}]},
            {"size": (40, 40), "objects": [
                {"what": "x = 3.5: round ties to even", "bbox": [3.5, 4.5, 10.0, 11.0], "segmentation": [[4, 5, 13, 6, 12, 15, 5, 14]]},
                {"what": "w < 0.5", "bbox": [20.0, 20.0, 0.3, 8.0], "segmentation": [_rect(18, 18, 24, 30)]},
                {"what": "crop cut by the picture's edge", "bbox": [30.0, 28.0, 15.0, 20.0],
                 "segmentation": [[28, 26, 44, 27, 43, 45, 29, 44]]}]},
            {"size": (200, 180), "objects": [
                {"what": "runs as a list", "bbox": [95.0, 22.0, 51.0, 37.0],
                 "segmentation": {"size": [180, 200], "counts": runs_of(list_mask)}},
                {"what": "compressed string with negative deltas", "bbox": [30.0, 40.0, 61.0, 101.0],
                 "segmentation": {"size": [180, 200], "counts": rle_to_string(ell_counts)}},
                {"what": "compressed string with a count >= 2^15", "bbox": [180.0, 0.0, 10.0, 180.0],
                 "segmentation": {"size": [180, 200], "counts": rle_to_string(big)}},
                {"what": "polygon of 24 vertices, crop larger than M", "bbox": [60.0, 85.0, 80.0, 70.0], "segmentation": [circle]},
                {"what": "crop smaller than M", "bbox": [10.0, 10.0, 5.0, 3.0], "segmentation": [_rect(9, 9, 14, 12.5)]}]},
        ],
    ]


def expected(batch, M):
    """The restatement over one batch of the table -> (masks (B, O + 1, M, M) int64 with the __image__ row of ones and zero
    padding rows, centres (B, O, 2) fp32 with the box-centre formula on the padding rows' box of -1, boxes (B, O, 4) fp32 with
    -1 padding)."""
    B, O = len(batch), max(len(s["objects"]) for s in batch)
    masks = np.zeros((B, O + 1, M, M), np.int64)
    masks[:, O] = 1
    boxes = np.full((B, O, 4), -1.0, f32)
    centres = np.zeros((B, O, 2), f32)
    for b, s in enumerate(batch):
        WW, HH = s["size"]
        for o, obj in enumerate(s["objects"]):
            boxes[b, o] = box_of(obj["bbox"], WW, HH)
            masks[b, o] = object_mask(obj["segmentation"], obj["bbox"], WW, HH, M)
        for o in range(O):
            centres[b, o] = centre_closed(boxes[b, o], masks[b, o])
    return masks, centres, boxes


def random_polygon(rng, WW, HH):
    """A seeded polygon for the property tests: 3 to 9 vertices, a quarter of them reaching outside the picture, coordinates
    on a grid of integers, halves or hundredths; sometimes a vertex is repeated.  Not sorted by angle, so they cross."""
    k = int(rng.integers(3, 10))
    margin = 6.0 if rng.random() < 0.25 else 0.0
    pts = np.stack([rng.uniform(-margin, WW + margin, k), rng.uniform(-margin, HH + margin, k)], 1)
    grid = (1.0, 0.5, 0.01)[int(rng.integers(0, 3))]
    pts = np.round(pts / grid) * grid
    if rng.random() < 0.2:
        j = int(rng.integers(0, k))
        pts = np.insert(pts, j, pts[j], axis=0)
    return [float(v) for v in pts.reshape(-1)]


# ------------------------------------------------------------------------------------------------ the folder
def write_folder(root, batch, split="train", first_id=101):
    """One batch of the table as <root>/MSCoco in the reference's layout: seeded PNG pictures of the table's sizes and the two
    annotation files with bbox and segmentation, the first object of a picture of several as an instance and the others as
    stuff -> image dir.  The dataset orders a picture's objects instances first, so the table's order is kept."""
    from PIL import Image
    base = os.path.join(root, "MSCoco")
    image_dir = os.path.join(base, "images", "%s2017" % split)
    os.makedirs(image_dir, exist_ok=True)
    os.makedirs(os.path.join(base, "annotations"), exist_ok=True)
    images, ann = [], {"instances": [], "stuff": []}
    for i, s in enumerate(batch):
        WW, HH = s["size"]
        image_id = first_id + i
        name = "%012d.png" % image_id
        px = np.random.default_rng(70 + image_id).integers(0, 256, size=(HH, WW, 3), dtype=np.uint8)
        Image.fromarray(px, "RGB").save(os.path.join(image_dir, name))
        images.append({"id": image_id, "file_name": name, "width": WW, "height": HH})
        for k, obj in enumerate(s["objects"]):
            instance = k == 0 and len(s["objects"]) > 1          # a picture without a stuff annotation is dropped
            ann["instances" if instance else "stuff"].append(
                {"id": image_id * 100 + k, "image_id": image_id, "category_id": 1 if instance else (3 + k % 2),
                 "bbox": list(obj["bbox"]), "segmentation": obj["segmentation"]})
    cats = {"instances": [{"id": 1, "name": "person"}, {"id": 2, "name": "dog"}],
            "stuff": [{"id": 3, "name": "grass"}, {"id": 4, "name": "sky"}]}
    for kind in ("instances", "stuff"):
        with open(os.path.join(base, "annotations", "%s_%s2017.json" % (kind, split)), "w") as f:
            json.dump({"images": images, "categories": cats[kind], "annotations": ann[kind]}, f)
    return image_dir
