"""The cases of csg_draw_graph_u8 (csrc/overlay.hip) and a numpy restatement of its pixel rule (include/csg_hip.h, DESIGN
4.10b).  Shared by test_sgdraw_cases.py (CPU: the restatement against bytes typed by hand) and test_gpu_sgdraw.py (the
kernel against the restatement, byte for byte).  The records are packed here by this file's own `seg`, `tri` and `node`,
from the header's description; the restatement is vectorised over pixels and loops over the primitives in ascending
order, so the highest record covering a pixel is the last to write it."""
import numpy as np

SEGMENT, TRIANGLE, NODE = 0, 1, 2
UNKNOWN = ord("?") - 32
WHITE, BLACK = (255, 255, 255), (0, 0, 0)
RED, GREEN, BLUE, PINK, SKY = (230, 25, 75), (60, 180, 75), (0, 130, 200), (255, 174, 185), (191, 239, 255)


def rgb(c):
    return c[0] | c[1] << 8 | c[2] << 16


def _i32(w):
    return w - (1 << 32) if w >= 1 << 31 else w


def seg(ax, ay, bx, by, colour, t=1):
    return [SEGMENT | t << 4, ax, ay, bx, by, 0, 0, rgb(colour)]


def tri(x0, y0, x1, y1, x2, y2, colour):
    return [TRIANGLE, x0, y0, x1, y1, x2, y2, rgb(colour)]


def node(x0, y0, x1, y1, fill, ink, r, text_off, n):
    return [_i32(NODE | r << 4 | rgb(ink) << 8), x0, y0, x1, y1, text_off, n, rgb(fill)]


def covers(rec, text, font, H, W):
    """One record -> (covered (H,W) bool, ink (H,W) bool), in int64."""
    rec = [int(v) for v in rec]
    kind, param = rec[0] & 15, (rec[0] >> 4) & 15
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    ink = np.zeros((H, W), bool)
    if kind == SEGMENT:
        ax, ay, bx, by = rec[1:5]
        dx, dy, vx, vy = bx - ax, by - ay, x - ax, y - ay
        L2, dot, cross = dx * dx + dy * dy, vx * dx + vy * dy, vx * dy - vy * dx
        t2 = param * param
        at_a = 4 * (vx * vx + vy * vy) <= t2
        at_b = 4 * ((x - bx) ** 2 + (y - by) ** 2) <= t2
        along = 4 * cross * cross <= t2 * L2
        if L2 == 0:
            return at_a, ink
        return np.where(dot <= 0, at_a, np.where(dot >= L2, at_b, along)), ink
    if kind == TRIANGLE:
        x0, y0, x1, y1, x2, y2 = rec[1:7]
        if (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) == 0:
            return ink.copy(), ink
        e0 = (x1 - x0) * (y - y0) - (y1 - y0) * (x - x0)
        e1 = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)
        e2 = (x0 - x2) * (y - y2) - (y0 - y2) * (x - x2)
        return ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)), ink
    assert kind == NODE, rec
    x0, y0, x1, y1, first, n = rec[1:7]
    if x1 < x0 or y1 < y0:
        return ink.copy(), ink
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    re = min(param, (x1 - x0) // 2, (y1 - y0) // 2)
    cx = np.where(x < x0 + re, x0 + re - x, np.where(x > x1 - re, x - (x1 - re), 0))
    cy = np.where(y < y0 + re, y0 + re - y, np.where(y > y1 - re, y - (y1 - re), 0))
    covered = inside & ~((cx > 0) & (cy > 0) & (cx * cx + cy * cy > re * re))
    tw = 6 * n - 1
    tx = x0 + max(0, (x1 - x0 + 1 - tw) // 2)
    ty = y0 + max(0, (y1 - y0 + 1 - 7) // 2)
    for k in range(n):
        byte = text[first + k]
        g = byte - 32 if 32 <= byte <= 126 else UNKNOWN
        for line in range(7):
            for bit in range(5):
                if (int(font[g][line]) >> (4 - bit)) & 1:
                    px, py = tx + 6 * k + bit, ty + line
                    if 0 <= px < W and 0 <= py < H and covered[py, px]:
                        ink[py, px] = True
    return covered, ink


def draw_graph(prims, prim_off, text, H, W, background, font):
    """-> uint8 (B,3,H,W): every picture starts as `background`; its records paint in ascending order."""
    B = len(prim_off) - 1
    out = np.empty((B, 3, H, W), np.uint8)
    out[:] = np.asarray(background, np.uint8)[None, :, None, None]
    for b in range(B):
        for rec in prims[prim_off[b]:prim_off[b + 1]]:
            covered, ink = covers(rec, text, font, H, W)
            fill, pen = int(rec[7]), (int(rec[0]) >> 8) & 0xffffff
            for ch in range(3):
                out[b, ch][covered] = (fill >> (8 * ch)) & 255
                out[b, ch][ink] = (pen >> (8 * ch)) & 255
    return out


def make_case(name, H, W, pictures, text=b"", background=WHITE):
    prims, off = [], [0]
    for p in pictures:
        prims += p
        off.append(len(prims))
    return {"name": "%dx%d %s" % (H, W, name), "H": H, "W": W, "prims": prims, "prim_off": off, "text": bytes(text),
            "background": background}


def capacity_case():
    """4096 records (the limit per picture) that all cross the one tile of a 16 x 16 canvas.  Record 0 is a node over the
    whole canvas; the 4095 above it never touch the columns 13 .. 15 apart from sixteen two-pixel nodes, so those columns
    are decided by the lowest record, after every other one was looked at: however long the kernel's list is, a list that
    drops what does not fit shows.  The two-pixel nodes sit on both sides of every power-of-two boundary from the top
    (records 4096 - 2^k - 1 and 4096 - 2^k share a pixel: the higher one must win)."""
    rng = np.random.default_rng(4096)
    prims = [node(-3, -3, 20, 20, SKY, BLACK, 0, 0, 0)]
    palette = (RED, GREEN, BLUE, PINK, BLACK)
    for i in range(1, 4096):
        kind = i % 3
        c = palette[i % 5]
        if kind == 0:       # a thin segment from the left of the canvas into it: its box crosses the tile
            prims.append(seg(int(rng.integers(-20, 0)), int(rng.integers(-8, 24)), int(rng.integers(0, 12)),
                             int(rng.integers(0, 16)), c, 1 + i % 2))
        elif kind == 1:     # a sliver of a triangle
            x, y = int(rng.integers(0, 10)), int(rng.integers(0, 15))
            prims.append(tri(x, y, x + 2, y, x - 30, y + int(rng.integers(-40, 40)), c))
        else:               # a small node, often partly above or left of the canvas
            x, y = int(rng.integers(-4, 9)), int(rng.integers(-4, 15))
            prims.append(node(x, y, x + 2, y + 1, c, WHITE, 1, 0, 0))
    for k in range(4, 12):                  # pairs around 4096 - 16, - 32, ... - 2048: a pass boundary for any such length
        hi = 4096 - (1 << k)
        y = k - 4
        prims[hi - 1] = node(13, y, 14, y, RED, BLACK, 0, 0, 0)
        prims[hi] = node(14, y, 15, y, GREEN, BLACK, 0, 0, 0)
    return make_case("4096 records across one tile", 16, 16, [prims])


def table():
    text = b"tileedgeaWide\x1f\x7f\xc8Mqg"
    T = {"tile": (0, 4), "edge": (4, 4), "a": (8, 1), "Wide": (9, 4), "???": (13, 3), "Mqg": (16, 3), "": (0, 0)}
    order = [node(2, 2, 12, 12, PINK, BLACK, 3, *T["a"]), seg(0, 0, 15, 15, BLUE, 3), tri(1, 14, 14, 14, 8, 4, GREEN)]
    cases = [
        make_case("horizontal, vertical and 45 degrees, t 1 2 3", 16, 16,
                  [[seg(2, 3, 13, 3, RED, 1), seg(4, 5, 4, 14, GREEN, 2), seg(6, 6, 12, 12, BLUE, 3)]]),
        make_case("shallow slope, discs of zero length, t 1 2 3 8", 16, 16,
                  [[seg(0, 2, 15, 5, RED, 1), seg(8, 10, 8, 10, GREEN, 8), seg(1, 8, 1, 8, BLUE, 1), seg(14, 8, 14, 8, BLACK, 2),
                    seg(2, 13, 2, 13, RED, 3), seg(15, 15, 3, 12, BLUE, 2)]]),
        make_case("t 8 and both ends outside", 16, 16,
                  [[seg(2, 13, 13, 2, PINK, 8), seg(-5, 7, 25, 9, BLACK, 2), seg(7, -30, 9, 40, RED, 1), seg(-9, -9, -2, -2, GREEN, 8)]]),
        # cross^2 reaches 7e15 here: int32 holds neither it nor t^2 L2
        make_case("the longest diagonals", 16, 16,
                  [[seg(-4096, -4096, 4096, 4096, RED, 1), seg(-4096, 4096, 4096, -4090, BLUE, 3),
                    seg(4096, 4090, -4096, -4096, GREEN, 8)]], background=(10, 200, 30)),
        make_case("triangles: both windings, degenerate, smallest, across the border", 12, 20,
                  [[tri(1, 1, 7, 1, 1, 7, RED), tri(18, 1, 12, 1, 18, 7, GREEN), tri(2, 9, 6, 9, 10, 9, BLACK),
                    tri(4, 4, 4, 4, 4, 4, BLACK), tri(9, 8, 10, 8, 9, 9, BLUE), tri(0, 0, -3, 1, 1, -3, BLACK),
                    tri(15, -3, 25, 6, 14, 8, PINK), tri(3, 15, 9, 10, 12, 14, SKY)]]),
        # 136 x 40: three tiles across (64, 64, 8) and three down (16, 16, 8); the primitives cross their borders
        make_case("across tile borders", 40, 136,
                  [[seg(-10, -5, 150, 45, RED, 3), seg(64, 0, 64, 39, GREEN, 2), seg(0, 16, 135, 16, BLUE, 1),
                    seg(63, 31, 128, 32, BLACK, 1), tri(60, 10, 70, 20, 58, 30, PINK), tri(120, 2, 140, 20, 126, 38, SKY),
                    node(50, 12, 80, 24, PINK, BLACK, 4, *T["tile"]), node(118, 28, 142, 45, SKY, RED, 8, *T["edge"]),
                    node(60, 30, 67, 33, GREEN, WHITE, 2, *T["Mqg"])]], text),
        make_case("nodes: one pixel, smaller than 2 r, r 0, no label", 16, 16,
                  [[node(3, 3, 3, 3, RED, BLACK, 0, *T[""]), node(6, 3, 6, 3, GREEN, WHITE, 8, *T["a"]),
                    node(9, 1, 13, 4, BLUE, WHITE, 8, *T[""]), node(1, 6, 9, 14, PINK, BLACK, 0, *T["a"]),
                    node(11, 7, 14, 15, SKY, BLACK, 8, *T[""]), node(12, 12, 11, 13, BLACK, BLACK, 0, *T[""])]], text),
        make_case("nodes clipped by each border, label wider and taller than the node", 12, 20,
                  [[node(-4, 3, 3, 8, PINK, BLACK, 3, *T["a"]), node(16, 2, 24, 10, SKY, BLACK, 4, *T["a"]),
                    node(6, -5, 12, 2, GREEN, BLACK, 2, *T["a"]), node(5, 9, 13, 16, RED, WHITE, 3, *T["a"]),
                    node(6, 4, 13, 8, BLUE, WHITE, 1, *T["Wide"])]], text),
        make_case("bytes 31, 127 and 200, and a lower node's ink under a higher node's fill", 16, 24,
                  [[node(1, 1, 22, 9, PINK, BLACK, 2, *T["???"]), node(2, 6, 21, 14, SKY, RED, 2, *T["Mqg"]),
                    node(8, 4, 12, 12, GREEN, BLACK, 1, *T[""])]], text),
        make_case("three pictures, one of them empty", 16, 16,
                  [[seg(1, 1, 14, 9, RED, 2), tri(2, 14, 12, 14, 7, 9, BLUE), node(8, 1, 15, 11, PINK, BLACK, 2, *T["a"])],
                   [],
                   [node(0, 0, 15, 15, SKY, BLACK, 8, *T["Mqg"]), seg(0, 15, 15, 0, GREEN, 1), seg(3, 3, 3, 3, RED, 3),
                    tri(15, 15, 9, 15, 15, 9, BLACK), node(5, 10, 9, 13, RED, WHITE, 0, *T[""])]], text, background=(10, 200, 30)),
        make_case("order: node, segment, triangle", 16, 16, [order], text),
        make_case("order: triangle, segment, node", 16, 16, [order[::-1]], text),
        capacity_case(),
    ]
    return cases


def expected(case, font):
    return draw_graph(case["prims"], case["prim_off"], case["text"], case["H"], case["W"], case["background"], font)
