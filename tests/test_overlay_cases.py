"""The numpy restatement of the box-outline rule (tests/overlay_cases.py) against bytes typed by hand, and the table of
cases against its own purpose.  No GPU."""
import numpy as np

import overlay_cases as oc


def test_the_restatement_reproduces_a_hand_written_8x8_picture():
    """8 x 8, thickness 1, a black picture.  Row 0 = (0.125, 0.125, 0.5, 0.5): x0 * 8 = 1, (x + w) * 8 = 5 -> columns and
    lines 1..4.  Row 1 = (0.375, 0.375, 0.625, 0.5): 0.375 * 8 = 3, clamp(1.0) * 8 = 8 -> columns 3..min(7, 7); lines
    3..(0.875 * 8 = 7) - 1 = 6.  Row 2 is __image__ with the whole frame as its box: not drawn.  Where the two outlines
    meet — (4, 3) and (3, 4) as (x, y) — the higher row wins; (4, 4) is inside row 1's rectangle but not on its outline,
    so row 0's corner stays."""
    a, b = 210, 220
    red = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                    [0, a, a, a, a, 0, 0, 0],
                    [0, a, 0, 0, a, 0, 0, 0],
                    [0, a, 0, b, b, b, b, b],
                    [0, a, a, b, a, 0, 0, b],
                    [0, 0, 0, b, 0, 0, 0, b],
                    [0, 0, 0, b, b, b, b, b],
                    [0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    img = np.zeros((1, 3, 8, 8), np.uint8)
    boxes = np.array([[[0.125, 0.125, 0.5, 0.5], [0.375, 0.375, 0.625, 0.5], [0, 0, 1, 1]]], np.float32)
    objs = np.array([[[4], [2], [oc.IMAGE_ID]]], np.int64)
    got = oc.draw_boxes(img, boxes, objs, oc.IMAGE_ID, oc.PALETTE, 1)
    assert np.array_equal(got[0, 0], red), got[0, 0]
    assert np.array_equal(got[0, 1], red + (red > 0)) and np.array_equal(got[0, 2], red + 2 * (red > 0))
    assert not img.any()                                              # the input is not written
    # thickness 2 fills row 0's 4 x 4 rectangle: every pixel of it is within 2 of a side
    got2 = oc.draw_boxes(img, boxes[:, :1], objs[:, :1], oc.IMAGE_ID, oc.PALETTE, 2)
    assert (got2[0, 0, 1:5, 1:5] == a).all() and int((got2[0, 0] == a).sum()) == 16


def test_pixel_rect_truncates_in_fp32():
    assert oc.pixel_rect([0.25, 0.25, 0.5, 0.5], 12, 20) == (5, 3, 14, 8)
    # fp32(0.35) * 20 is 7.0 in fp32 and 6.99999988 in fp64
    assert float(np.float32(0.35)) * 20 < 7 and oc.pixel_rect([0.35, 0.0, 0.05, 0.25], 12, 20)[0] == 7
    assert oc.pixel_rect([1.25, 0.25, 0.5, 0.5], 16, 16) == (15, 4, 15, 11)            # wholly right of the frame: its edge
    assert oc.pixel_rect([-0.5, 0.0, 0.75, 1.0], 16, 16) == (0, 0, 3, 15)
    assert oc.pixel_rect([0.5, 0.5, 1 / 20, 1 / 12], 12, 20) == (10, 6, 10, 6)
    assert oc.pixel_rect([float("-inf"), 0.0, float("inf"), 1.0], 8, 8) == (0, 0, 0, 7)     # NaN sum clamps to 0
    for skipped in ([-1, -1, -1, -1], [0.1, float("nan"), 0.2, 0.2], [0.1, 0.1, 0.0, 0.2], [0.1, 0.1, 0.2, -0.2]):
        assert oc.pixel_rect(skipped, 16, 16) is None
    assert oc.pixel_rect([-1, -1, -1, 0.5], 16, 16) is None and oc.pixel_rect([-1, -1, 0.5, 0.5], 16, 16) == (0, 0, 0, 0)


def test_every_case_paints_something_except_the_all_skipped_one():
    cases = oc.table()
    assert len(cases) == 2 * 2 * 5 + 3
    assert {(c["H"], c["W"]) for c in cases} == {(16, 16), (12, 20)} and {c["thickness"] for c in cases} == {1, 2}
    for c in cases:
        assert c["img"].shape == (2, 3, c["H"], c["W"]) and c["boxes"].shape == (2, 5, 4) and len(c["palette"]) == 3
        want = oc.expected(c)
        changed = (want != c["img"]).any(axis=1)
        if c["kind"] == "all skipped":
            assert not changed.any(), c["name"]
            continue
        assert changed[0].any() and changed[1].any(), c["name"]
        # the __image__ row's whole-frame box and the padded row are not drawn: the frame's corner pixel keeps its bytes
        # unless a drawn row reaches it
        without = dict(c, boxes=c["boxes"].copy())
        without["boxes"][:, 4] = -1
        special = (oc.expected(without) != want).any(axis=(1, 2, 3))
        drawn = c["kind"] in ("beyond 1", "at x = 0", "one pixel", "x * W an integer", "fp32 product")
        assert special.all() if drawn else not special.any(), (c["name"], special)
        # rows 1 and 4 share palette[1] (4 % 3): the wrap is exercised whenever row 4 is drawn
        if c["kind"] == "one pixel":
            assert int((oc.expected(without) != want).any(axis=1).sum()) == 2          # one pixel per sample
