"""Scene-graph pictures on the host (no GPU): the numpy restatement of csg_draw_graph_u8's pixel rule (tests/sgdraw_cases.py)
against pictures typed by hand, the conditions a laid-out graph must meet (canonicalsg2im_amd/sgdraw.py) on the fixture's
twelve graphs and at each refusal boundary, and the host refusals of `ops.draw_graph_u8`."""
import numpy as np
import pytest

import sgdraw_cases as sc
from conftest import load_golden
from test_authored_graphs import fixture_vocab


def _font():
    from canonicalsg2im_amd.font5x7 import FONT
    return FONT


def _typed(rows, colours):
    """A picture typed as characters -> uint8 (3,H,W)."""
    return np.asarray([[colours[ch] for ch in row] for row in rows], np.uint8).transpose(2, 0, 1)


KEY = {".": sc.WHITE, "#": sc.BLACK, "o": sc.PINK, "r": sc.RED}


# --------------------------------------------------------------------------------------------- 1. the restatement
def test_restatement_draws_a_thin_diagonal_and_two_discs_as_typed():
    prims = [sc.seg(1, 1, 6, 6, sc.BLACK, 1), sc.seg(1, 5, 1, 5, sc.RED, 2), sc.seg(5, 1, 5, 1, sc.RED, 3)]
    got = sc.draw_graph(prims, [0, 3], b"", 8, 8, sc.WHITE, _font())
    assert np.array_equal(got[0], _typed(["....rrr.",
                                          ".#..rrr.",
                                          "..#.rrr.",
                                          "...#....",
                                          ".r..#...",
                                          "rrr..#..",
                                          ".r....#.",
                                          "........"], KEY))


def test_restatement_fills_a_triangle_of_either_winding_with_its_border_as_typed():
    want = _typed(["........",
                   ".######.",
                   ".#####..",
                   ".####...",
                   ".###....",
                   ".##.....",
                   ".#......",
                   "........"], KEY)
    for t in (sc.tri(1, 1, 6, 1, 1, 6, sc.BLACK), sc.tri(1, 1, 1, 6, 6, 1, sc.BLACK)):
        assert np.array_equal(sc.draw_graph([t], [0, 1], b"", 8, 8, sc.WHITE, _font())[0], want)
    none = sc.draw_graph([sc.tri(1, 1, 3, 3, 6, 6, sc.BLACK)], [0, 1], b"", 8, 8, sc.WHITE, _font())
    assert (none == 255).all()


def test_restatement_draws_a_rounded_7_by_9_node_with_one_letter_as_typed():
    got = sc.draw_graph([sc.node(2, 1, 8, 9, sc.PINK, sc.BLACK, 2, 1, 1)], [0, 1], b"xT", 12, 12, sc.WHITE, _font())
    assert np.array_equal(got[0], _typed(["............",
                                          "....ooo.....",
                                          "...#####....",
                                          "..ooo#ooo...",
                                          "..ooo#ooo...",
                                          "..ooo#ooo...",
                                          "..ooo#ooo...",
                                          "..ooo#ooo...",
                                          "...oo#oo....",
                                          "....ooo.....",
                                          "............",
                                          "............"], KEY))
    # a byte without a glyph draws '?', and a label wider than its node is cut at the node's border
    q = sc.draw_graph([sc.node(0, 0, 6, 8, sc.PINK, sc.BLACK, 0, 0, 1)], [0, 1], b"\xc8", 12, 12, sc.WHITE, _font())
    assert np.array_equal(q, sc.draw_graph([sc.node(0, 0, 6, 8, sc.PINK, sc.BLACK, 0, 0, 1)], [0, 1], b"?", 12, 12, sc.WHITE, _font()))
    cut = sc.draw_graph([sc.node(1, 1, 4, 5, sc.PINK, sc.BLACK, 0, 0, 2)], [0, 1], b"TT", 12, 12, sc.WHITE, _font())
    assert np.array_equal(cut[0], _typed(["............",
                                          ".####.......",
                                          ".oo#o.......",
                                          ".oo#o.......",
                                          ".oo#o.......",
                                          ".oo#o.......",
                                          "............"] + ["............"] * 5, KEY))


def test_the_highest_record_decides_and_the_table_is_what_it_says():
    font = _font()
    cases = {c["name"]: c for c in sc.table()}
    assert len(cases) == 13
    a = sc.expected(cases["16x16 order: node, segment, triangle"], font)[0]
    b = sc.expected(cases["16x16 order: triangle, segment, node"], font)[0]
    assert not np.array_equal(a, b)
    assert tuple(a[:, 11, 8]) == sc.GREEN and tuple(b[:, 11, 8]) == sc.PINK           # triangle over node; node over both
    assert tuple(a[:, 3, 3]) == sc.BLUE and tuple(b[:, 3, 3]) == sc.PINK              # segment over node; node over it
    three = cases["16x16 three pictures, one of them empty"]
    assert three["prim_off"] == [0, 3, 3, 8]
    assert (sc.expected(three, font)[1] == np.asarray((10, 200, 30), np.uint8)[:, None, None]).all()
    # the longest diagonal: int32 would wrap, and a wrapped rule paints another picture
    d = sc.expected(cases["16x16 the longest diagonals"], font)[0]
    assert all(tuple(d[:, i, i]) == sc.GREEN for i in range(16)) and tuple(d[:, 0, 15]) == (10, 200, 30)
    cap = cases["16x16 4096 records across one tile"]
    assert cap["prim_off"] == [0, 4096]
    e = sc.expected(cap, font)[0]
    assert tuple(e[:, 12, 15]) == sc.SKY                                              # only record 0 reaches that pixel
    for k in range(4, 12):
        assert tuple(e[:, k - 4, 13]) == sc.RED and tuple(e[:, k - 4, 14]) == sc.GREEN == tuple(e[:, k - 4, 15])
    # the cases' own packing is the package's
    from canonicalsg2im_amd import ops
    assert ops.graph_segment(1, -2, 3, 4, sc.RED, 5) == sc.seg(1, -2, 3, 4, sc.RED, 5)
    assert ops.graph_triangle(1, 2, 3, 4, -5, 6, sc.BLUE) == sc.tri(1, 2, 3, 4, -5, 6, sc.BLUE)
    assert ops.graph_node(1, 2, 3, 4, sc.PINK, sc.WHITE, 8, 9, 10) == sc.node(1, 2, 3, 4, sc.PINK, sc.WHITE, 8, 9, 10)


# --------------------------------------------------------------------------------------------- 2. the layout
@pytest.fixture(scope="module")
def fx():
    meta, _ = load_golden("authored_graphs")
    return meta, fixture_vocab(meta)


def _decode(prims):
    segs = [p for p in prims if p[0] & 15 == sc.SEGMENT]
    heads = [p for p in prims if p[0] & 15 == sc.TRIANGLE]
    nodes = [p for p in prims if p[0] & 15 == sc.NODE]
    return segs, heads, nodes


def _check_layout(width, height, prims, text, n_objects, n_edges, style):
    """The conditions every laid-out picture meets."""
    segs, heads, nodes = _decode(prims)
    assert all(isinstance(v, int) for p in prims for v in p)
    assert width % 4 == 0 and 0 < width <= 2048 and 0 < height <= 2048 and len(prims) <= 4096
    assert [p[0] & 15 for p in prims] == [sc.SEGMENT] * len(segs) + [sc.TRIANGLE] * len(heads) + [sc.NODE] * len(nodes)
    assert len(segs) == len(heads) == 2 * n_edges and len(nodes) == n_objects + n_edges
    rects = np.asarray([p[1:5] for p in nodes], np.int64).reshape(-1, 4)
    x0, y0, x1, y1 = rects.T
    assert (x0 >= 0).all() and (y0 >= 0).all() and (x1 < width).all() and (y1 < height).all()
    apart = (x1[:, None] < x0[None, :]) | (x1[None, :] < x0[:, None]) | (y1[:, None] < y0[None, :]) | (y1[None, :] < y0[:, None])
    assert (apart | np.eye(len(nodes), dtype=bool)).all(), "two nodes intersect"
    for p in nodes:                                          # the whole label fits, and lies inside the text
        n = p[6]
        assert 0 <= p[5] and p[5] + n <= len(text)
        assert p[3] - p[1] + 1 >= 6 * n - 1 and p[4] - p[2] + 1 >= 7
    font = _font()

    def on_border(x, y, p):
        """(x, y) is a pixel of node p's outline that the node covers (not cut away by a rounded corner)."""
        covered = sc.covers([p[0], p[1] - p[1], p[2] - p[2], p[3] - p[1], p[4] - p[2], 0, 0, p[7]], b"", font,
                            p[4] - p[2] + 1, p[3] - p[1] + 1)[0]
        inside = p[1] <= x <= p[3] and p[2] <= y <= p[4]
        return inside and (x in (p[1], p[3]) or y in (p[2], p[4])) and bool(covered[y - p[2], x - p[1]])

    objects, preds = nodes[:n_objects], nodes[n_objects:]
    for e in range(n_edges):
        pred = preds[e]
        for k, (src, dst) in ((2 * e, (None, pred)), (2 * e + 1, (pred, None))):
            s, h = segs[k], heads[k]
            ax, ay, bx, by = s[1:5]
            assert (h[1], h[2]) == (bx, by), "the head's tip is the segment's end"
            assert abs((h[3] - h[1]) * (h[6] - h[2]) - (h[4] - h[2]) * (h[5] - h[1])) > 0, "a degenerate head"
            starts = [src] if src is not None else objects
            ends = [dst] if dst is not None else objects
            assert any(p[1] <= ax <= p[3] and p[2] <= ay <= p[4] for p in starts), "an arrow starts outside its source"
            assert any(on_border(bx, by, p) for p in ends), "an arrow's tip is not on its target's border"
            assert s[7] == h[7] and (s[0] >> 4) & 15 == style["thickness"]
    return rects


def test_layout_of_the_fixture_graphs_meets_every_condition_and_repeats(fx):
    from canonicalsg2im_amd import authored, sgdraw
    meta, vocab = fx
    graphs = authored.load_graphs(meta["graphs"], vocab)
    names = authored.object_labels(graphs)
    rows = authored.encode_graphs(graphs, vocab)[1].tolist()
    st = sgdraw.DEFAULT_STYLE
    assert st["object_fill"] == (255, 174, 185) and st["predicate_fill"] == (191, 239, 255)        # lightpink1, lightblue1
    drawn_types = [st["types"][k] for k in (sgdraw.ORIGINAL, sgdraw.TRANSITIVE, sgdraw.SYMMETRIC)]
    assert len(set(drawn_types)) == 3 and st["types"][sgdraw.ORIGINAL] == (st["edge"], st["predicate_fill"])
    skip = {vocab["pred_name_to_idx"][n] for n in ("__in_image__", "__padding__")}
    for g, graph in enumerate(graphs):
        n = len(graph["objects"])
        edges = [r for r in rows[g] if r[1] not in skip]
        assert names[g][n] is None and len(edges) > 0
        w, h, prims, text = sgdraw.layout_graph(names[g], rows[g], vocab["pred_idx_to_name"])
        assert (w, h, prims, text) == sgdraw.layout_graph(names[g], rows[g], vocab["pred_idx_to_name"])
        _check_layout(w, h, prims, text, n, len(edges), st)
        _, _, nodes = _decode(prims)
        assert all(p[7] == sc.rgb(st["object_fill"]) for p in nodes[:n])
        assert all(p[7] == sc.rgb(st["predicate_fill"]) for p in nodes[n:])
        assert [text[p[5]:p[5] + p[6]].decode() for p in nodes[:n]] == names[g][:n]
        assert [text[p[5]:p[5] + p[6]].decode() for p in nodes[n:]] == [vocab["pred_idx_to_name"][r[1]] for r in edges]
        # with edge types: the same places, the types' colours on the arrows and the predicate nodes
        types = [k % 4 for k in range(len(rows[g]))]
        w2, h2, typed, text2 = sgdraw.layout_graph(names[g], rows[g], vocab["pred_idx_to_name"], types)
        assert (w2, h2, text2) == (w, h, text) and [p[1:7] for p in typed] == [p[1:7] for p in prims]
        _check_layout(w2, h2, typed, text2, n, len(edges), st)
        kinds = [types[k] for k, r in enumerate(rows[g]) if r[1] not in skip]
        segs, heads, nodes = _decode(typed)
        for e, kind in enumerate(kinds):
            arrow, fill = st["types"][kind]
            assert {segs[2 * e][7], segs[2 * e + 1][7], heads[2 * e][7], heads[2 * e + 1][7]} == {sc.rgb(arrow)}
            assert nodes[n + e][7] == sc.rgb(fill)
    # the batch: records back to back, label offsets rebased into one text; a flat-form graph beside the fixture's
    sizes, prims, off, text = sgdraw.layout_batch(graphs, vocab)
    assert len(sizes) == 12 and off[0] == 0 and off[-1] == len(prims) and len(off) == 13
    for g in range(12):
        w, h, mine, own = sgdraw.layout_graph(names[g], rows[g], vocab["pred_idx_to_name"])
        assert sizes[g] == (w, h)
        for p, q in zip(prims[off[g]:off[g + 1]], mine):
            assert p[:5] == q[:5] and p[7] == q[7]
            if p[0] & 15 == sc.NODE:
                assert text[p[5]:p[5] + p[6]] == own[q[5]:q[5] + q[6]]


def test_layout_of_a_flat_graph_wraps_into_two_rows_and_draws_self_relations():
    from canonicalsg2im_amd import sgdraw
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("vg")
    preds = vocab["pred_idx_to_name"]
    rel = vocab["pred_name_to_idx"]["__left of__"]
    names = ["object name %d" % i for i in range(12)] + [None]
    rows = [[i, rel, (i + 5) % 12] for i in range(12)] + [[3, rel, 3]] + [[i, vocab["pred_name_to_idx"]["__in_image__"], 12]
                                                                          for i in range(12)]
    w, h, prims, text = sgdraw.layout_graph(names, rows, preds)
    rects = _check_layout(w, h, prims, text, 12, 13, sgdraw.DEFAULT_STYLE)
    assert len(set(rects[:12, 1].tolist())) == 2                                      # two rows of objects
    one = dict(sgdraw.DEFAULT_STYLE, wrap_width=4096)
    w1, h1, prims1, text1 = sgdraw.layout_graph(names, rows, preds, style=one)
    rects1 = _check_layout(w1, h1, prims1, text1, 12, 13, one)
    assert len(set(rects1[:12, 1].tolist())) == 1 and w1 > w and h1 < h


def test_layout_refuses_a_picture_beyond_each_limit_and_accepts_the_limit_itself():
    from canonicalsg2im_amd import sgdraw
    preds = ["__in_image__", "left", "__padding__"]
    one = dict(sgdraw.DEFAULT_STYLE, wrap_width=1 << 20)
    # width: fourteen labels of 20 letters and one of 13 end at 2047, rounded up to 2048; one of 14 gives 2056
    w, h, prims, text = sgdraw.layout_graph(["x" * 20] * 14 + ["y" * 13], [], preds, style=one)
    assert (w, h) == (2048, 8 + 15 + 8) and len(prims) == 15
    _check_layout(w, h, prims, text, 15, 0, one)
    with pytest.raises(ValueError, match=r"scene graph 7: the picture's width would be 2056, at most 2048"):
        sgdraw.layout_graph(["x" * 20] * 14 + ["y" * 14], [], preds, style=one, index=7)
    # height: every triplet between the same two objects takes a line of its own, 23 pixels each: 47 + 23 * 87 = 2048
    w, h, prims, text = sgdraw.layout_graph(["a", "b"], [[0, 1, 1]] * 87, preds)
    assert h == 2048
    _check_layout(w, h, prims, text, 2, 87, sgdraw.DEFAULT_STYLE)
    with pytest.raises(ValueError, match=r"scene graph 0: the picture's height would be 2071, at most 2048"):
        sgdraw.layout_graph(["a", "b"], [[0, 1, 1]] * 88, preds)
    # primitives: five per triplet and one per object: 816 triplets among sixteen objects are 4096, 817 are 4101
    names = ["x" * 18] * 16
    pairs = [[s, 1, o] for s in range(16) for o in range(16)]
    rows = (pairs * 4)[:817]
    w, h, prims, text = sgdraw.layout_graph(names, rows[:816], preds, style=one)
    assert len(prims) == 4096
    _check_layout(w, h, prims, text, 16, 816, one)
    with pytest.raises(ValueError, match=r"scene graph 3: the picture's primitives would be 4101, at most 4096"):
        sgdraw.layout_graph(names, rows, preds, style=one, index=3)
    with pytest.raises(ValueError, match=r"scene graph 0: triplet 0 has the type 9"):
        sgdraw.layout_graph(["a", "b"], [[0, 1, 1]], preds, [9])


# --------------------------------------------------------------------------------------------- 3. host refusals
def test_draw_graph_u8_refuses_on_the_host_what_the_rule_cannot_hold():
    """Every refusal fires before a device is asked for: this test runs without one."""
    from canonicalsg2im_amd import ops
    ok = [sc.seg(0, 0, 4096, -4096, sc.RED, 8), sc.tri(0, 0, 1, 1, 2, 0, sc.RED), sc.node(0, 0, 5, 5, sc.RED, sc.BLACK, 8, 1, 3)]
    rec, off = ops.check_graph_records(ok, [0, 1, 3], 4)
    assert rec.dtype == off.dtype and tuple(rec.shape) == (3, 8) and off.tolist() == [0, 1, 3]
    assert ops.check_graph_records([], [0, 0], 0)[0].shape == (0, 8)
    full = [sc.seg(0, 0, 1, 1, sc.RED, 1)] * 4096
    assert ops.check_graph_records(full + ok, [0, 4096, 4099], 4)[0].shape == (4099, 8)

    def refused(match, prims, off=None, text=b"abcd"):
        with pytest.raises(ValueError, match=match):
            ops.draw_graph_u8(prims, [0, len(prims)] if off is None else off, text, 16, 16, sc.WHITE)

    refused(r"picture 1 has 4097 primitives, at most 4096", ok + full + full[:1], [0, 3, 4100])
    refused(r"picture 0, primitive 0: a coordinate outside \[-4096, 4096\]", [sc.seg(0, 4097, 1, 1, sc.RED, 1)])
    refused(r"picture 0, primitive 1: a coordinate outside", [ok[0], sc.tri(0, 0, 1, 1, 2, -4097, sc.RED)])
    refused(r"picture 1, primitive 0: a coordinate outside", [ok[0], sc.node(-4097, 0, 5, 5, sc.RED, sc.BLACK, 0, 0, 0)], [0, 1, 2])
    refused(r"thickness t outside 1 \.\. 8", [sc.seg(0, 0, 1, 1, sc.RED, 0)])
    refused(r"thickness t outside 1 \.\. 8", [sc.seg(0, 0, 1, 1, sc.RED, 9)])
    refused(r"corner radius r outside 0 \.\. 8", [sc.node(0, 0, 5, 5, sc.RED, sc.BLACK, 9, 0, 0)])
    refused(r"label range outside the 4 bytes of text", [sc.node(0, 0, 5, 5, sc.RED, sc.BLACK, 0, 2, 3)])
    refused(r"label range outside the 4 bytes of text", [sc.node(0, 0, 5, 5, sc.RED, sc.BLACK, 0, -1, 1)])
    refused(r"label range outside the 0 bytes of text", [sc.node(0, 0, 5, 5, sc.RED, sc.BLACK, 0, 0, 1)], text=b"")
    refused(r"unknown kind", [[3, 0, 0, 0, 0, 0, 0, 0]])
    refused(r"prim_off must be B \+ 1 ascending offsets", ok, [0, 2])
    refused(r"prim_off must be B \+ 1 ascending offsets", ok, [0, 2, 1, 3])
    refused(r"prim_off must be B \+ 1 ascending offsets", ok, [1, 3])
    # a node's label words are not coordinates: an offset beyond 4096 into a long text is fine
    long_text = b"x" * 5000
    assert ops.check_graph_records([sc.node(0, 0, 40, 10, sc.RED, sc.BLACK, 0, 4990, 10)], [0, 1], len(long_text))[0].shape == (1, 8)


def test_command_line_refuses_the_flag_without_scene_graphs():
    from canonicalsg2im_amd.scripts import sample
    with pytest.raises(SystemExit, match="--draw_scene_graphs 1 needs --scene_graphs"):
        sample.parse_args(["--draw_scene_graphs", "1"])
    with pytest.raises(SystemExit):
        sample.parse_args(["--draw_scene_graphs", "3"])
    assert sample.parse_args([]).draw_scene_graphs == 0
    assert "--draw_scene_graphs" in sample.__doc__ and "--split and --layouts" in sample.__doc__
