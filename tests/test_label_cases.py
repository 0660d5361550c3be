"""CPU checks of the label pictures' host side: the numpy restatement of csg_draw_labels_u8's pixel rule
(tests/label_cases.py) against bytes typed by hand, the font table, the two helpers that name the objects
(authored.object_labels, authored.labels_from_objs) and the command line's refusal.  The kernel itself is held to the
restatement in test_gpu_labels.py."""
import itertools

import numpy as np
import pytest
import torch

import label_cases as lc
from canonicalsg2im_amd.font5x7 import FONT


def _planes(pattern, values, ink=0):
    return np.stack([np.array([[ink if ch == "#" else v for ch in row] for row in pattern], np.uint8) for v in values])


# --------------------------------------------------------------------------------------------- 1. the restatement
def test_restatement_draws_an_I_in_an_8x8_box_as_typed():
    # the box is the picture: the strip is lines 0..7 (nine lines clipped to eight), tw = 5, rw = 8, tx = 0 + 3 // 2 = 1
    img = np.full((1, 3, 8, 8), 100, np.uint8)
    boxes = np.array([[[0.0, 0.0, 1.0, 1.0]]], np.float32)
    objs = np.array([[[1]]], np.int64)
    got = lc.draw_labels(img, boxes, objs, 0, np.array([[200, 100, 50]], np.uint8), [["I"]], FONT)
    red = np.array([[150, 150, 150, 150, 150, 150, 150, 150],        # (100 + 200 + 1) >> 1 = 150
                    [150, 150, 0, 0, 0, 150, 150, 150],
                    [150, 150, 150, 0, 150, 150, 150, 150],
                    [150, 150, 150, 0, 150, 150, 150, 150],
                    [150, 150, 150, 0, 150, 150, 150, 150],
                    [150, 150, 150, 0, 150, 150, 150, 150],
                    [150, 150, 150, 0, 150, 150, 150, 150],
                    [150, 150, 0, 0, 0, 150, 150, 150]], np.uint8)
    pattern = ["........", "..###...", "...#....", "...#....", "...#....", "...#....", "...#....", "..###..."]
    assert np.array_equal(got[0, 0], red)
    assert np.array_equal(got[0], _planes(pattern, (150, 100, 75)))   # (100 + 100 + 1) >> 1 = 100, (100 + 50 + 1) >> 1 = 75
    assert np.array_equal(img, np.full((1, 3, 8, 8), 100, np.uint8))


def test_restatement_clips_the_strip_at_py1_and_cuts_the_text_at_px1_as_typed():
    # columns 2..8, lines 3..5 of a 8 x 12 picture: "HH" is 11 wide in 7 columns, so tx = px0 and the second H keeps its
    # first column alone; three lines hold the strip's top line and the glyph rows 0 and 1
    H, W = 8, 12
    img = np.full((1, 3, H, W), 40, np.uint8)
    boxes = np.array([[lc._box(W, H, 2, 3, 8, 5)]], np.float32)
    assert lc.oc.pixel_rect(boxes[0, 0], H, W) == (2, 3, 8, 5)
    objs = np.array([[[7]]], np.int64)
    got = lc.draw_labels(img, boxes, objs, 0, np.array([[210, 211, 212]], np.uint8), [["HH"]], FONT)
    pattern = ["            ",
               "            ",
               "            ",
               "  .......   ",
               "  #...#.#   ",
               "  #...#.#   ",
               "            ",
               "            "]
    want = np.stack([np.array([[0 if ch == "#" else v if ch == "." else 40 for ch in row] for row in pattern], np.uint8)
                     for v in (125, 126, 126)])                        # (40 + 210 + 1) >> 1, (40 + 211 + 1) >> 1, (40 + 212 + 1) >> 1
    assert np.array_equal(got[0], want)


def test_table_covers_what_it_says():
    cases = lc.table()
    assert sorted({(c["H"], c["W"]) for c in cases}) == [(16, 16), (24, 40)]
    assert all(c["img"].shape[0] == 2 and c["boxes"].shape[1] == 5 and int(c["img"].max()) < int(c["palette"].min()) for c in cases)
    for c in cases:
        want = lc.expected(c, FONT)
        none = [[None] * 5] * 2
        assert np.array_equal(lc.draw_labels(c["img"], c["boxes"], c["objs"], 0, c["palette"], none, FONT), c["img"])
        assert (want != c["img"]).any(), c["name"]
        # `__image__` (row 2) and the all -1 row (row 3) carry labels and change nothing
        bare = [[l if o not in (2, 3) else None for o, l in enumerate(row)] for row in c["labels"]]
        assert np.array_equal(lc.draw_labels(c["img"], c["boxes"], c["objs"], 0, c["palette"], bare, FONT), want), c["name"]


# --------------------------------------------------------------------------------------------- 2. the font
def test_font_table():
    assert FONT.shape == (95, 7) and FONT.dtype == np.uint8
    assert not (FONT & 0xE0).any()
    assert not FONT[0].any()
    assert all(FONT[g].any() for g in range(1, 95))
    for a, b in itertools.combinations(range(95), 2):
        assert not np.array_equal(FONT[a], FONT[b]), (chr(32 + a), chr(32 + b))
    assert FONT[ord("I") - 32].tolist() == [0b01110, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110]
    with pytest.raises(ValueError):
        FONT[0, 0] = 1                                                 # the table is not to be written


# --------------------------------------------------------------------------------------------- 3. the names
def test_object_labels_of_both_authored_forms():
    from canonicalsg2im_amd.authored import object_labels
    cube = {"shape": "cube", "color": "red", "material": "metal", "size": "large"}
    ball = {"shape": "sphere", "color": "blue", "material": "rubber", "size": "small"}
    graphs = [{"objects": [cube, ball, cube], "relationships": {"right": [[], [0], [1]]}},
              {"objects": [ball], "relationships": {"right": [[]]}}]
    assert object_labels(graphs) == [["cube, red, metal, large", "sphere, blue, rubber, small", "cube, red, metal, large", None],
                                     ["sphere, blue, rubber, small", None, None, None]]
    flat = [{"objects": ["person", "grass"], "relationships": [[0, "left of", 1]]},
            {"objects": ["tree", "sky", "person"], "relationships": []}]
    assert object_labels(flat) == [["person", "grass", None, None], ["tree", "sky", "person", None]]


def test_object_labels_rows_are_the_rows_of_encode_graphs():
    from canonicalsg2im_amd import authored
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    vocab["pred_name_to_idx"].setdefault("__padding__", len(vocab["pred_name_to_idx"]))
    vocab["pred_name_to_idx"].setdefault("__in_image__", len(vocab["pred_name_to_idx"]))
    graphs = [{"objects": ["obj_1", "obj_2", "obj_3"], "relationships": []}, {"objects": ["obj_4"], "relationships": []}]
    objs, _, counts = authored.encode_graphs(graphs, vocab)
    labels = authored.object_labels(graphs)
    assert [len(row) for row in labels] == [objs.shape[1]] * 2 and counts.tolist() == [4, 2]
    assert labels == authored.labels_from_objs(objs, vocab)


def test_labels_from_objs_one_attribute_and_four():
    from canonicalsg2im_amd.authored import labels_from_objs
    from canonicalsg2im_amd.synth import make_vocab
    tiny = make_vocab("tiny")
    objs = torch.tensor([[[3], [1], [0], [0]], [[6], [0], [0], [0]]], dtype=torch.int64)
    assert labels_from_objs(objs, tiny) == [["obj_3", "obj_1", None, None], ["obj_6", None, None, None]]
    assert labels_from_objs(objs.numpy(), tiny) == labels_from_objs(objs, tiny)
    clevr = make_vocab("clevr")
    assert list(clevr["attributes"]) == ["shape", "color", "material", "size"]
    objs = torch.tensor([[[2, 8, 1, 2], [1, 3, 2, 1], [0, 0, 0, 0]]], dtype=torch.int64)
    assert labels_from_objs(objs, clevr) == [["shape_2, color_8, material_1, size_2", "shape_1, color_3, material_2, size_1", None]]
    with pytest.raises(ValueError, match="name no object"):
        labels_from_objs(torch.tensor([[[2, 99, 1, 2]]]), clevr)


# --------------------------------------------------------------------------------------------- 4. the packing, the command
def test_pack_labels_offsets_and_bytes():
    from canonicalsg2im_amd import ops
    packed, head = ops.pack_labels([["ab", None, ""], ["é", b"\xc8\n", "xyz"]], 2, 3)
    assert head == 4 * 7 and packed.dtype == torch.uint8
    assert packed[:head].view(torch.int32).tolist() == [0, 2, 2, 2, 3, 5, 8]
    assert bytes(packed[head:head + 8].tolist()) == b"ab?\xc8\nxyz" and packed.numel() > head + 8
    for bad in (["ab"], [["a", "b", "c"]], [["a", "b"], ["c", "d"]], "ab", [["a", "b", 3], ["c", "d", "e"]]):
        with pytest.raises(RuntimeError, match="draw_labels_u8"):
            ops.pack_labels(bad, 2, 3)


def test_command_line_refuses_labels_without_boxes():
    from canonicalsg2im_amd.scripts import sample as cli
    with pytest.raises(SystemExit, match=r"--draw_labels.*--draw_boxes"):
        cli.parse_args(["--draw_labels", "1", "--draw_boxes", "0"])
    args = cli.parse_args([])
    assert args.draw_labels == 0 and args.draw_boxes == 1
    assert cli.parse_args(["--draw_labels", "1"]).draw_labels == 1
