"""Pictures of scene graphs: the host layout of `ops.draw_graph_u8` (csg_draw_graph_u8).

The reference draws a graph with GraphViz (sg2im/vis.py:draw_scene_graph, img_%06d_sg.png of scripts/run_model.py): every
object a node, every triplet a predicate node of its own, two arrows s -> predicate -> o.  Here the same picture is laid
out on the host as an ARC DIAGRAM in integers, and painted on the device in one launch:

  * the objects sit in one row in the order of the graph, or in two rows (the first half above) when one row would be
    wider than style["wrap_width"];
  * the predicate node of a triplet sits at the horizontal midpoint of its two ends, on the first free line below the
    objects, found greedily in the order of the triplets;
  * an arrow is a segment with a triangle at its end: from the middle of the subject's lower side to the predicate's upper
    side a quarter of its width towards the subject, and from the quarter towards the object to the middle of the
    object's lower side — it starts on its source node and has its tip on its target's border, clear of rounded corners;
  * the records go out as segments, then arrowheads, then nodes, so that lines pass under nodes.

Nothing is random, every coordinate is an integer, no two nodes intersect and every node holds its whole label.  The
`__image__` row, `__in_image__` rows and padding rows are not drawn.  With `edge_types` (one `triplet_type` per row) an
edge and its predicate node are coloured by type: original, transitive and converse edges are told apart, which shows
the canonical graph the model was given.
"""
from math import isqrt

from . import ops

ORIGINAL, TRANSITIVE, SYMMETRIC, ANTI_SYMMETRIC = 0, 1, 2, 3            # triplet_type (sg2im/data/base_dataset.py)

DEFAULT_STYLE = {
    "background": (255, 255, 255),
    "ink": (0, 0, 0),                        # every label
    "object_fill": (255, 174, 185),          # the reference's lightpink1
    "predicate_fill": (191, 239, 255),       # the reference's lightblue1: predicate nodes without edge types
    "edge": (0, 0, 0),                       # arrows without edge types
    # triplet_type -> (arrow, predicate fill): original as above, transitive green, converse (both kinds) orange
    "types": {ORIGINAL: ((0, 0, 0), (191, 239, 255)), TRANSITIVE: ((34, 139, 34), (193, 255, 193)),
              SYMMETRIC: ((205, 102, 0), (255, 218, 185)), ANTI_SYMMETRIC: ((205, 102, 0), (255, 218, 185))},
    "thickness": 1, "radius": 4,             # of the arrows' lines; of the nodes' corners
    "pad_x": 4, "pad_y": 4,                  # between a label and its node's border
    "margin": 8,                             # between the nodes and the picture's border
    "gap_x": 12, "gap_y": 8,                 # between neighbouring nodes of a line; between lines
    "row_gap": 24,                           # between the objects and the first line of predicates (room for the heads)
    "head_length": 7, "head_half_width": 3,
    "wrap_width": 1024,
}

MAX_SIDE = 2048                   # csg_draw_graph_u8's canvas limit
MAX_PRIMS = ops.GRAPH_MAX_PRIMS


def _label(name):
    return name if isinstance(name, bytes) else str(name).encode("ascii", errors="replace")


def _rdiv(a, b):
    """a / b rounded to the nearest integer, halves up, in integers (b > 0)."""
    return (2 * a + b) // (2 * b)


def _arrow(sx, sy, tx, ty, colour, style):
    """-> (segment record, head record) of the arrow S -> T with its tip at T."""
    dx, dy = tx - sx, ty - sy
    length = max(1, isqrt(dx * dx + dy * dy))
    hl, hw = style["head_length"], style["head_half_width"]
    bx, by = tx - _rdiv(dx * hl, length), ty - _rdiv(dy * hl, length)            # the middle of the head's base
    ox, oy = _rdiv(-dy * hw, length), _rdiv(dx * hw, length)
    return (ops.graph_segment(sx, sy, tx, ty, colour, style["thickness"]),
            ops.graph_triangle(tx, ty, bx + ox, by + oy, bx - ox, by - oy, colour))


def layout_graph(names, rows, pred_names, edge_types=None, style=DEFAULT_STYLE, index=0):
    """One graph -> (width, height, primitives, text): the records of `ops.draw_graph_u8` (segments, then heads, then nodes)
    with label offsets into `text`, on a canvas of width x height, width % 4 == 0.  names: the objects' labels in row
    order, None for rows that are not drawn (`__image__`, padding: authored.object_labels); rows: [s, p, o] triplets;
    pred_names: the vocabulary's pred_idx_to_name; edge_types: one triplet_type per row, or None for one colour.  A picture
    beyond 2048 in either direction or 4096 primitives raises ValueError("scene graph <index>: ...")."""
    st = style
    node_h = 7 + 2 * st["pad_y"]
    text = bytearray()
    nodes = []                               # (x0, y0, x1, y1, fill, text_off, n)

    def node_w(label):
        return max(6 * len(label) - 1, 1) + 2 * st["pad_x"]

    # ---- the objects: one row, or two
    drawn = [i for i, name in enumerate(names) if name is not None]
    labels = {i: _label(names[i]) for i in drawn}
    one_row = sum(node_w(labels[i]) for i in drawn) + st["gap_x"] * max(len(drawn) - 1, 0) + 2 * st["margin"]
    first = len(drawn) if one_row <= st["wrap_width"] else (len(drawn) + 1) // 2
    rect = {}
    y, right = st["margin"], 0
    for line in (drawn[:first], drawn[first:]):
        if not line:
            continue
        x = st["margin"]
        for i in line:
            w = node_w(labels[i])
            rect[i] = (x, y, x + w - 1, y + node_h - 1)
            x += w + st["gap_x"]
        right = max(right, x - st["gap_x"] - 1)
        y += node_h + st["gap_y"]
    base = y - st["gap_y"] + st["row_gap"]   # the first line of predicates
    for i in drawn:
        nodes.append(rect[i] + (st["object_fill"], len(text), len(labels[i])))
        text += labels[i]

    # ---- the predicates: the midpoint of the two ends, the first free line
    lines, segments, heads, preds = [], [], [], []
    for k, (s, p, o) in enumerate(rows):
        s, p, o = int(s), int(p), int(o)
        name = pred_names[p]
        if name in ("__in_image__", "__padding__") or s not in rect or o not in rect:
            continue
        colour, fill = st["edge"], st["predicate_fill"]
        if edge_types is not None:
            kind = int(edge_types[k])
            if kind not in st["types"]:
                raise ValueError("scene graph %d: triplet %d has the type %d, the style lists %s" % (
                    index, k, kind, sorted(st["types"])))
            colour, fill = st["types"][kind]
        label = _label(name)
        w = node_w(label)
        mid = ((rect[s][0] + rect[s][2]) // 2 + (rect[o][0] + rect[o][2]) // 2) // 2
        x0 = max(st["margin"], mid - w // 2)
        x1 = x0 + w - 1
        for taken in lines:
            if all(x1 + st["gap_x"] < a or b + st["gap_x"] < x0 for a, b in taken):
                break
        else:
            taken = []
            lines.append(taken)
        taken.append((x0, x1))
        y0 = base + (node_h + st["gap_y"]) * next(j for j, t in enumerate(lines) if t is taken)
        right = max(right, x1)
        preds.append((x0, y0, x1, y0 + node_h - 1, fill, len(text), len(label)))
        text += label
        # the arrow from s arrives a quarter of the node towards s, the one to o leaves a quarter towards o, both clear of
        # the rounded corners
        cs, co = (rect[s][0] + rect[s][2]) // 2, (rect[o][0] + rect[o][2]) // 2
        quarter = w // 4 if cs <= co else -(w // 4)
        clear = min(st["radius"], (w - 1) // 2, (node_h - 1) // 2)
        arrive = min(max((x0 + x1) // 2 - quarter, x0 + clear), x1 - clear)
        leave = min(max((x0 + x1) // 2 + quarter, x0 + clear), x1 - clear)
        for (ax, ay), (bx, by) in (((cs, rect[s][3]), (arrive, y0)), ((leave, y0), (co, rect[o][3]))):
            seg, head = _arrow(ax, ay, bx, by, colour, st)
            segments.append(seg)
            heads.append(head)
    nodes += preds

    width = (right + 1 + st["margin"] + 3) // 4 * 4
    height = (base + (node_h + st["gap_y"]) * len(lines) - st["gap_y"] if lines else base - st["row_gap"]) + st["margin"]
    count = len(segments) + len(heads) + len(nodes)
    for what, got, most in (("width", width, MAX_SIDE), ("height", height, MAX_SIDE), ("primitives", count, MAX_PRIMS)):
        if got > most:
            raise ValueError("scene graph %d: the picture's %s would be %d, at most %d" % (index, what, got, most))
    prims = segments + heads + [ops.graph_node(x0, y0, x1, y1, fill, st["ink"], st["radius"], off, n)
                                for x0, y0, x1, y1, fill, off, n in nodes]
    return width, height, prims, bytes(text)


def layout_batch(graphs, vocab, triplets=None, triplet_type=None, style=DEFAULT_STYLE):
    """B authored graphs -> (sizes [(width, height)], primitives, prim_off, text) for one `ops.draw_graph_u8` call: the
    pictures' records back to back with their label offsets rebased into one text.  Host only.  triplets (B,T,3) and
    triplet_type (B,T), lists or CPU tensors: the edges and their types; without them the host-encoded rows of
    authored.encode_graphs in one colour."""
    from . import authored
    names = authored.object_labels(graphs)
    if triplets is None:
        if triplet_type is not None:
            raise ValueError("draw_scene_graphs: triplet_type needs triplets")
        triplets = authored.encode_graphs(graphs, vocab)[1]
    triplets = triplets.tolist() if hasattr(triplets, "tolist") else triplets
    if triplet_type is not None:
        triplet_type = triplet_type.tolist() if hasattr(triplet_type, "tolist") else triplet_type
    if len(triplets) != len(graphs) or (triplet_type is not None and len(triplet_type) != len(graphs)):
        raise ValueError("draw_scene_graphs: %d graphs, but triplets for %d" % (len(graphs), len(triplets)))
    sizes, prims, prim_off, text = [], [], [0], b""
    for g in range(len(graphs)):
        w, h, mine, label_bytes = layout_graph(names[g], triplets[g], vocab["pred_idx_to_name"],
                                               None if triplet_type is None else triplet_type[g], style, index=g)
        for rec in mine:
            if rec[0] & 15 == ops.GRAPH_NODE:
                rec[5] += len(text)
        sizes.append((w, h))
        prims += mine
        prim_off.append(len(prims))
        text += label_bytes
    return sizes, prims, prim_off, text


def draw_canvas(graphs, vocab, device, triplets=None, triplet_type=None, style=DEFAULT_STYLE):
    """-> (canvas uint8 (B, 3, max h, max w) on `device`, sizes [(width, height)]): one packed upload, one launch.  Device
    `triplets` / `triplet_type` are read back in one copy (the call's only synchronisation)."""
    import torch
    if triplets is not None and triplet_type is not None and getattr(triplets, "is_cuda", False) \
            and getattr(triplet_type, "is_cuda", False):
        both = torch.cat([triplets, triplet_type.unsqueeze(-1).to(triplets.dtype)], dim=-1).cpu()
        triplets, triplet_type = both[..., :3], both[..., 3]
    elif getattr(triplets, "is_cuda", False):
        triplets = triplets.cpu()
    sizes, prims, prim_off, text = layout_batch(graphs, vocab, triplets, triplet_type, style)
    canvas = ops.draw_graph_u8(prims, prim_off, text, max(h for _, h in sizes), max(w for w, _ in sizes), style["background"],
                               device=device)
    return canvas, sizes


def draw_scene_graphs(graphs, vocab, device, triplets=None, triplet_type=None, style=DEFAULT_STYLE):
    """B authored graphs -> a list of B uint8 (3, h_b, w_b) device tensors, each a cropped view of one canvas painted in one
    launch.  Without `triplets` the edges are the host-encoded rows of authored.encode_graphs (what graphs.json lists), in
    one colour; with `triplets` (B,T,3) / `triplet_type` (B,T) — what `Sampler.generate_from_graphs(return_graph=True)`
    returns — they are the canonical graph the model was given, coloured by type."""
    canvas, sizes = draw_canvas(graphs, vocab, device, triplets, triplet_type, style)
    return [canvas[b, :, :h, :w] for b, (w, h) in enumerate(sizes)]
