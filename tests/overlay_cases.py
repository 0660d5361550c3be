"""The box-outline cases of csg_draw_boxes_u8 (csrc/overlay.hip) and a numpy restatement of its pixel rule (DESIGN 4.10b,
include/csg_hip.h).  Shared by test_overlay_cases.py (CPU: the restatement against bytes typed by hand) and
test_gpu_authored.py (the kernel against the restatement, byte for byte)."""
import itertools

import numpy as np

F = np.float32
IMAGE_ID = 0
PALETTE = np.array([[210, 211, 212], [220, 221, 222], [230, 231, 232]], np.uint8)       # P = 3: o % P wraps at O = 5


def clamp01(v):
    return (v if v < F(1) else F(1)) if v > F(0) else F(0)          # a NaN (-inf + inf) gives 0


def pixel_rect(box, H, W):
    """(px0, py0, px1, py1) of an xywh box in fp32, one rounding per operation, or None for a row that is not drawn."""
    x, y, w, h = (F(v) for v in box)
    if all(v == F(-1) for v in (x, y, w, h)) or any(v != v for v in (x, y, w, h)) or w <= 0 or h <= 0:
        return None
    with np.errstate(invalid="ignore"):
        x0, x1, y0, y1 = clamp01(x), clamp01(F(x + w)), clamp01(y), clamp01(F(y + h))
    px0 = min(W - 1, int(F(x0 * F(W))))
    px1 = max(px0, min(W - 1, int(F(x1 * F(W))) - 1))
    py0 = min(H - 1, int(F(y0 * F(H))))
    py1 = max(py0, min(H - 1, int(F(y1 * F(H))) - 1))
    return px0, py0, px1, py1


def draw_boxes(img, boxes, objs, image_id, palette, thickness):
    """img uint8 (B,3,H,W), boxes (B,O,4), objs (B,O,A), palette uint8 (P,3) -> a new uint8 (B,3,H,W).  Rows ascending, so
    a pixel on several outlines ends with the colour of the highest row."""
    out = img.copy()
    B, _, H, W = img.shape
    for b in range(B):
        for o in range(boxes.shape[1]):
            rect = None if objs[b, o, 0] == image_id else pixel_rect(boxes[b, o], H, W)
            if rect is None:
                continue
            px0, py0, px1, py1 = rect
            for y in range(py0, py1 + 1):
                for x in range(px0, px1 + 1):
                    if min(x - px0, px1 - x, y - py0, py1 - y) < thickness:
                        out[b, :, y, x] = palette[o % len(palette)]
    return out


NAN = float("nan")
# the fifth row of a sample, per special kind, as a function of (H, W): (sample 0's, sample 1's)
SPECIAL = {
    "zero width": lambda H, W: ([0.25, 0.25, 0.0, 0.5], [0.1, 0.1, 0.5, -0.25]),
    "nan": lambda H, W: ([0.25, NAN, 0.5, 0.5], [NAN, NAN, NAN, NAN]),
    "beyond 1": lambda H, W: ([0.5, 0.625, 0.9, 1.5], [1.25, 0.25, 0.5, 0.5]),
    "at x = 0": lambda H, W: ([0.0, 0.25, 0.3, 0.45], [-0.5, 0.0, 0.75, 1.0]),
    "one pixel": lambda H, W: ([0.5, 0.5, 1.0 / W, 1.0 / H], [0.0, 0.0, 1.0 / W, 1.0 / H]),
}


def make_case(H, W, thickness, kind, rows=None, seed=0):
    """One table row: B = 2, O = 5, A = 2; the rows of a sample are a plain box, a box that overlaps it, `__image__` (with
    a box that WOULD be drawn), an all -1 padded row (with an object id that WOULD be drawn), and the special row."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    img = rng.integers(0, 200, size=(2, 3, H, W), dtype=np.uint8)              # below every palette byte
    boxes = np.array([[[0.125, 0.125, 0.5, 0.5], [0.375, 0.3, 0.5, 0.45], [0.0, 0.0, 1.0, 1.0], [-1, -1, -1, -1], [0, 0, 0, 0]],
                      [[0.3, 0.05, 0.4, 0.9], [0.05, 0.4, 0.9, 0.25], [0.0, 0.0, 1.0, 1.0], [-1, -1, -1, -1], [0, 0, 0, 0]]],
                     np.float32)
    objs = np.array([[[3, 1], [1, 2], [IMAGE_ID, 0], [2, 1], [1, 1]]] * 2, np.int64)
    if rows is not None:
        boxes[:] = np.asarray(rows, np.float32)
    else:
        s0, s1 = SPECIAL[kind](H, W)
        boxes[0, 4], boxes[1, 4] = s0, s1
    return {"name": "%dx%d t%d %s" % (H, W, thickness, kind), "H": H, "W": W, "thickness": thickness, "kind": kind,
            "img": img, "boxes": boxes, "objs": objs, "palette": PALETTE, "image_id": IMAGE_ID}


def table():
    cases = [make_case(H, W, t, kind) for (H, W), t, kind in
             itertools.product(((16, 16), (12, 20)), (1, 2), SPECIAL)]
    # x * W lands on an integer in fp32: 0.25 * 20 = 5 and 0.75 * 20 = 15 exactly -> columns 5..14, not 4 or 15
    exact = [[0.25, 0.25, 0.5, 0.5], [0.25, 0.5, 0.5, 0.25], [0, 0, 1, 1], [-1, -1, -1, -1], [0.75, 0.0, 0.25, 0.25]]
    cases.append(make_case(12, 20, 1, "x * W an integer", rows=[exact, exact]))
    # fp32(0.35) * 20 rounds UP to 7.0 in fp32 (in fp64 the product is 6.9999999 -> 6): the product is one fp32 operation
    rounded = [[0.35, 0.25, 0.3, 0.5], [0.1, 0.1, 0.2, 0.2], [0, 0, 1, 1], [-1, -1, -1, -1], [0.35, 0.0, 0.05, 0.25]]
    cases.append(make_case(12, 20, 1, "fp32 product", rows=[rounded, rounded]))
    # nothing is drawn: __image__ ids, padding, NaN, no width, no height
    skipped = [[0.1, 0.1, 0.5, 0.5], [-1, -1, -1, -1], [0.2, NAN, 0.5, 0.5], [0.2, 0.2, 0.0, 0.5], [0.2, 0.2, 0.5, -0.1]]
    c = make_case(16, 16, 2, "all skipped", rows=[skipped, skipped])
    c["objs"][:, 0, 0] = IMAGE_ID
    cases.append(c)
    return cases


def expected(case):
    return draw_boxes(case["img"], case["boxes"], case["objs"], case["image_id"], case["palette"], case["thickness"])
