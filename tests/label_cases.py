"""The label cases of csg_draw_labels_u8 (csrc/overlay.hip) and a numpy restatement of its pixel rule (DESIGN 4.10b,
include/csg_hip.h).  Shared by test_label_cases.py (CPU: the restatement against bytes typed by hand) and
test_gpu_labels.py (the kernel against the restatement, byte for byte).  The pixel rectangle is overlay_cases.pixel_rect,
the outline rule's own."""
import numpy as np

import overlay_cases as oc

IMAGE_ID = oc.IMAGE_ID
PALETTE = oc.PALETTE                     # P = 3: o % P wraps at O = 5; every byte above the pictures' (< 200)
UNKNOWN = ord("?") - 32


def label_bytes(label):
    """A label as the bytes the kernel sees: None and "" none, a str as ASCII with errors="replace", bytes as they are."""
    if not label:
        return b""
    return label if isinstance(label, bytes) else label.encode("ascii", errors="replace")


def draw_labels(img, boxes, objs, image_id, palette, labels, font):
    """img uint8 (B,3,H,W), boxes (B,O,4), objs (B,O,A), palette uint8 (P,3), labels B x O, font uint8 (95,7) -> a new uint8
    (B,3,H,W).  Rows ascending and every row computed from the INPUT picture, so a pixel in several strips ends as the
    highest row alone made it."""
    out = img.copy()
    B, _, H, W = img.shape
    for b in range(B):
        for o in range(boxes.shape[1]):
            text = label_bytes(labels[b][o])
            rect = None if objs[b, o, 0] == image_id or not text else oc.pixel_rect(boxes[b, o], H, W)
            if rect is None:
                continue
            px0, py0, px1, py1 = rect
            tw, rw = 6 * len(text) - 1, px1 - px0 + 1
            tx = px0 + max(0, (rw - tw) // 2)
            colour = palette[o % len(palette)].astype(np.int64)
            for y in range(py0, min(py1, py0 + 8) + 1):
                for x in range(px0, px1 + 1):
                    r, c = y - py0 - 1, x - tx
                    ink = False
                    if 0 <= r <= 6 and 0 <= c < tw and c % 6 < 5:
                        byte = text[c // 6]
                        g = byte - 32 if 32 <= byte <= 126 else UNKNOWN
                        ink = bool((int(font[g][r]) >> (4 - c % 6)) & 1)
                    out[b, :, y, x] = 0 if ink else (img[b, :, y, x].astype(np.int64) + colour + 1) >> 1
    return out


def _box(W, H, px0, py0, px1, py1):
    """An xywh box whose pixel rectangle is exactly (px0, py0, px1, py1): corners half a pixel inside, so that no fp32
    rounding of x * W decides a column."""
    return [(px0 + 0.5) / W, (py0 + 0.5) / H, (px1 - px0 + 1) / W, (py1 - py0 + 1) / H]


def make_case(name, H, W, rects, labels, seed=0):
    """One table row: B = 2, O = 5, A = 2, pictures below every palette byte as overlay_cases.make_case draws them.  `rects`
    and `labels`: per sample five rows; a rect is (px0, py0, px1, py1), None for an all -1 row, or a list of four floats
    taken as the box itself.  Row 2 of every sample carries `__image__`."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    img = rng.integers(0, 200, size=(2, 3, H, W), dtype=np.uint8)
    boxes = np.zeros((2, 5, 4), np.float32)
    for b in range(2):
        for o in range(5):
            r = rects[b][o]
            boxes[b, o] = [-1, -1, -1, -1] if r is None else (r if isinstance(r, list) else _box(W, H, *r))
    objs = np.array([[[3, 1], [1, 2], [IMAGE_ID, 0], [2, 1], [1, 1]]] * 2, np.int64)
    case = {"name": "%dx%d %s" % (H, W, name), "H": H, "W": W, "img": img, "boxes": boxes, "objs": objs, "palette": PALETTE,
            "image_id": IMAGE_ID, "labels": labels}
    for b in range(2):                          # the table's own premise: the boxes land where the row says
        for o in range(5):
            if isinstance(rects[b][o], tuple):
                assert oc.pixel_rect(boxes[b, o], H, W) == rects[b][o], (case["name"], b, o)
    return case


FULL = (0, 0, 39, 23)


def table():
    far = (30, 14, 39, 23)            # a corner box that touches no other row's strip
    cases = [
        # "ab" is 11 wide: in 21 columns the slack is 10 (tx = px0 + 5), in 20 columns 9 (tx = px0 + 4, not 5)
        make_case("even and odd slack", 24, 40,
                  [[(2, 1, 22, 12), (2, 13, 21, 23), FULL, None, (24, 1, 38, 10)],
                   [(0, 0, 10, 9), (12, 0, 23, 9), FULL, None, (26, 2, 37, 12)]],
                  [["ab", "ab", "image", "pad", "x"], ["ab", "ab", "image", "pad", "y"]]),
        # "abc" is 17 wide: one more than a box of 16 columns; "a much longer name" is cut after a few letters
        make_case("text wider than the box", 24, 40,
                  [[(3, 2, 18, 14), (20, 2, 35, 14), FULL, None, (5, 15, 30, 23)],
                   [(0, 0, 15, 10), (16, 0, 20, 10), FULL, None, (22, 12, 27, 23)]],
                  [["abc", "a much longer name", "image", "pad", "the text is cut off at the right side"],
                   ["abc", "wide", "image", "pad", "Wq"]]),
        # three lines high: the strip is the whole box, the glyphs lose their lower rows; one line high: no glyph row at all
        make_case("a box 3 lines high", 24, 40,
                  [[(4, 5, 30, 7), (4, 10, 30, 10), FULL, None, (4, 14, 30, 21)],
                   [(0, 21, 20, 23), (22, 20, 39, 23), FULL, None, (10, 2, 30, 10)]],
                  [["gjpqy", "line", "image", "pad", "nine"], ["low", "edge", "image", "pad", "Top"]]),
        # the strip and the text run into the last column and the last line
        make_case("right and bottom border", 24, 40,
                  [[(28, 3, 39, 15), (20, 17, 39, 23), FULL, None, (0, 18, 12, 23)],
                   [(33, 0, 39, 8), (0, 16, 39, 23), FULL, None, (36, 12, 39, 23)]],
                  [["right", "corner", "image", "pad", "bot"], ["R", "bottom line", "image", "pad", "|"]]),
        # row 1's strip lies over the ink of row 0, row 4's over both; the lower rows' ink must not show through
        make_case("overlapping strips", 24, 40,
                  [[(4, 4, 34, 20), (10, 6, 30, 18), FULL, None, (14, 8, 28, 16)],
                   [(0, 0, 39, 23), (0, 2, 39, 12), FULL, None, (0, 4, 39, 14)]],
                  [["MMMMM", "WWW", "image", "pad", "##"], ["HHHHHH", "EEEEEE", "image", "pad", "888888"]]),
        # "" and None on drawable boxes: no strip either; `__image__` and the all -1 row carry labels and are not drawn
        make_case("empty, None, __image__ and padding", 24, 40,
                  [[(2, 2, 20, 14), (22, 2, 38, 14), FULL, None, far],
                   [(2, 2, 20, 14), (22, 2, 38, 14), FULL, None, far]],
                  [["", None, "image", "pad", "ok"], [None, "", "image", "pad", ""]]),
        # a byte of 200 and one of 10 draw '?'; so does a character outside ASCII, replaced on the host
        make_case("bytes without a glyph", 24, 40,
                  [[(1, 1, 25, 11), (1, 12, 25, 23), FULL, None, (27, 1, 39, 11)],
                   [(1, 1, 25, 11), (1, 12, 25, 23), FULL, None, (27, 1, 39, 11)]],
                  [[b"a\xc8b", b"a\nb", "image", "pad", "é"], ["a?b", b"\x7f\x1f", "image", "pad", b"\xff"]]),
        make_case("one character", 24, 40,
                  [[(5, 5, 5, 20), (8, 5, 12, 20), FULL, None, (15, 5, 21, 20)],
                   [(0, 0, 4, 8), (35, 0, 39, 8), FULL, None, (17, 10, 22, 18)]],
                  [["i", "j", "image", "pad", "k"], ["l", "m", "image", "pad", "n"]]),
        # boxes given as numbers: beyond 1.0, at x = 0 with a negative corner, NaN, no width (overlay_cases.SPECIAL)
        make_case("boxes of the outline table", 24, 40,
                  [[[0.5, 0.625, 0.9, 1.5], [-0.5, 0.0, 0.75, 1.0], [0.0, 0.0, 1.0, 1.0], None, [0.25, oc.NAN, 0.5, 0.5]],
                   [[0.35, 0.25, 0.3, 0.5], [0.25, 0.25, 0.0, 0.5], [0.0, 0.0, 1.0, 1.0], None, [0.1, 0.1, 0.5, -0.25]]],
                  [["out", "left", "image", "pad", "nan"], ["fp32", "flat", "image", "pad", "neg"]]),
    ]
    small = (0, 0, 15, 15)
    cases += [
        make_case("even and odd slack", 16, 16,
                  [[(1, 0, 13, 8), (2, 9, 13, 15), small, None, (14, 9, 15, 15)],
                   [(0, 0, 6, 6), (8, 0, 15, 6), small, None, (0, 8, 15, 15)]],
                  [["ab", "ab", "image", "pad", "."], ["a", "b", "image", "pad", "ab"]]),
        make_case("cut, clipped and overlapping", 16, 16,
                  [[(0, 0, 15, 15), (4, 1, 11, 3), small, None, (2, 2, 15, 15)],
                   [(5, 13, 15, 15), (0, 0, 10, 9), small, None, (6, 4, 15, 12)]],
                  [["sixteen", "Ay", "image", "pad", "x" * 40], ["end", "ab", "image", "pad", b"\xc8\n"]]),
    ]
    return cases


def expected(case, font):
    return draw_labels(case["img"], case["boxes"], case["objs"], case["image_id"], case["palette"], case["labels"], font)
