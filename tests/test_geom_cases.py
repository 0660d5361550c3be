"""The geometry matrix on the CPU (tests/geom_cases.py): `geom_ref64` against the oracle's boxes_to_layout /
masks_to_layout (pinned to the reference by tests/golden) and against F.grid_sample with autograd, both in float64; every
row's distance from the discontinuities of the box / mask gradients and of the painter's compositing; and the table's
coverage of every kernel, dispatch branch and corner, computed from the restated launch rules."""
import pytest
import torch

import geom_cases as gc
from geom_cases import CASES, case_ids

RUN = [c for c in CASES if not c["refuse"]]
LAYOUT = [c for c in RUN if c["family"] == "layout"]


def _agree(c, ref, other, what):
    assert set(ref) == set(other), sorted(set(ref) ^ set(other))
    for name, r in ref.items():
        if r is None:
            assert other[name] is None, name
            continue
        assert other[name] is not None and tuple(r.shape) == tuple(other[name].shape), name
        scale = float(r.abs().max()) if r.numel() else 0.0
        err = float((r - other[name]).abs().max()) if r.numel() else 0.0
        assert err <= 1e-10 * scale + 1e-300, "%s %s vs %s: %.3e of scale %.3e" % (c["name"], name, what, err, scale)


@pytest.mark.parametrize("c", LAYOUT, ids=case_ids(LAYOUT))
def test_ref64_against_oracle(c):
    """Outputs and every requested gradient of every layout row: geom_ref64 against oracle.boxes_to_layout /
    masks_to_layout (train mode and test_mode) evaluated in float64, to 1e-10 of each tensor's scale."""
    d = gc.make_data(c)
    _agree(c, gc.geom_ref64(c, d), gc.evaluate(c, d, gc.ORACLE, torch.float64), "oracle")


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_ref64_against_grid_sample(c):
    """Every row: geom_ref64 against torch.nn.functional.grid_sample on the reference's own sampling grids, in float64 with
    autograd (paint rows: grid_sample's mask samples, composited by lowest mass rank)."""
    d = gc.make_data(c)
    _agree(c, gc.geom_ref64(c, d), gc.evaluate(c, d, gc.GRID_SAMPLE, torch.float64), "grid_sample")


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_rows_keep_clear_of_discontinuities(c):
    """Judged on the reference alone.  (a) every contributing sample coordinate has the same floor() in float32 (ATen's
    order) as in float64; paint rows: (b) the valid objects' masses of one image are pairwise more than 1e-3 apart,
    relative, and (c) no sampled mask value lies within 1e-4 of 0.5.  A row that fails moves its seed."""
    d = gc.make_data(c)
    assert gc.floor_mismatches(c, d) == 0, c["name"]
    if c["entry"] == "layout_paint":
        gap, thr = gc.paint_margins(c, d)
        assert gap > gc.PAINT_MASS_GAP, "%s: two masses %.3e apart" % (c["name"], gap)
        assert thr > gc.PAINT_THRESHOLD_GAP, "%s: a sample %.3e from the threshold" % (c["name"], thr)


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_float32_arithmetic_leaves_room_under_the_gate(c):
    """The device test holds outputs, vecs and image gradients to 1e-5 of the scale.  A row whose float32 CPU oracle is
    itself beyond 7e-6 there tests the number format, not the kernel (pixel centres and sample coordinates carry n * 2^-24
    of rounding however they are computed): such a row changes its geometry or data, as the table explains where it did."""
    d = gc.make_data(c)
    ref, f32 = gc.geom_ref64(c, d), gc.evaluate(c, d, gc.ORACLE, torch.float32)
    for name, r in ref.items():
        if r is None or not r.numel() or name in ("dboxes", "dmasks"):
            continue
        scale, err = float(r.abs().max()), float((f32[name].double() - r).abs().max())
        assert err <= 7e-6 * scale + 1e-6, "%s %s: the float32 oracle is %.2e of the scale off" % (c["name"], name, err / scale)


CROPS = [c for c in RUN if c["family"] == "crop"]


@pytest.mark.parametrize("c", CROPS, ids=case_ids(CROPS))
def test_crop_oracle_is_the_pinned_one(c):
    """The float32 oracle of the crop rows is oracle.crop_objects itself; in float32 it and grid_sample on this file's
    grids are the same arithmetic: crops and box gradients bit for bit, the image gradient up to the order in which
    autograd adds the crops of one image (1e-6 of its scale)."""
    d = gc.make_data(c)
    a = gc.evaluate(c, d, gc.ORACLE, torch.float32)
    b = gc.evaluate(c, d, gc.GRID_SAMPLE, torch.float32)
    for name in a:
        assert (a[name] is None) == (b[name] is None), name
        if a[name] is not None:
            err = float((a[name] - b[name]).abs().max()) if a[name].numel() else 0.0
            assert err <= (1e-6 * float(a[name].abs().max()) if name == "dimg" else 0.0), (c["name"], name, err)


def test_box_families_are_what_they_say():
    for c in RUN:
        d = gc.make_data(c)
        bx = d["boxes"].reshape(-1, 4)
        n = c["W"] if c["family"] == "crop" else (c["masks"][1] if c["masks"] else 8)
        assert bool((bx[:, 2:] != 0).all()), c["name"]
        x0, y0, w, h = bx.unbind(1)
        if c["boxes"] == "inside":
            assert bool(((bx[:, :2] > 0) & (bx[:, :2] + bx[:, 2:] < 1) & (bx[:, 2:] > 0)).all()), c["name"]
        if c["boxes"] == "full":
            assert bool((bx == torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=bx.dtype)).all())
        if c["boxes"] in ("border", "mixed"):
            assert bool((x0 < 0).any() and (x0 + w > 1).any() and (y0 < 0).any() and (y0 + h > 1).any()), c["name"]
        if c["boxes"] in ("reversed", "mixed"):
            assert bool((w < 0).any()), c["name"]
        if c["boxes"] in ("outside", "mixed"):
            off = (torch.maximum(x0, x0 + w * (1 + 0.5 / n)) < 0) | (torch.minimum(x0, x0 - w * 0.5 / n) > 1)
            assert bool(off.any()) and (c["boxes"] == "mixed" or bool(off.all())), c["name"]
        if c["boxes"] in ("thin", "mixed"):
            if c["family"] == "crop":
                s = gc.crop_slopes(c, d)
                assert bool(((s[:, 0] > 0) & (s[:, 0] < 1e-3)).any() and ((s[:, 1] > 0) & (s[:, 1] < 1e-3)).any()), c["name"]
            else:
                assert bool((torch.isclose(w * (c["W"] - 1), torch.tensor(0.3, dtype=w.dtype), rtol=1e-5)).any()), c["name"]
                assert bool((torch.isclose(h * (c["H"] - 1), torch.tensor(0.3, dtype=w.dtype), rtol=1e-5)).any()), c["name"]


def test_outside_boxes_contribute_exact_zeros():
    for c in RUN:
        if c["boxes"] != "outside":
            continue
        ref = gc.geom_ref64(c, gc.make_data(c))
        for name, r in ref.items():
            if r is not None and (name != "dimg" or c["family"] == "crop"):
                assert float(r.abs().max()) == 0.0, (c["name"], name)


def _rows(cases=RUN, **kw):
    return [c for c in cases if all((v(c[k]) if callable(v) else c[k] == v) for k, v in kw.items())]


def _levels(cases):
    """[(row, level index, (h, w), rule)] of the layout rows that launch the sum kernels"""
    return [(c, i, c["sizes"][i], r) for c in cases for i, r in enumerate(gc.level_rules(c))]


def test_table_covers_every_kernel_branch_and_corner():
    names = case_ids()
    assert len(set(names)) == len(names)
    for c in CASES:
        assert c["kernels"] == gc._kernel_names(c), c["name"]
    assert {c["entry"] for c in RUN} == {"layout_pyramid", "disc_input", "layout_paint", "abi_slice", "crop_objects"}
    lay = [c for c in LAYOUT if c["entry"] != "layout_paint"]
    lv = _levels(lay)
    box = [t for t in lv if t[0]["masks"] is None]
    # ---- forward: both kernels, both thread maps, the S values, the widths and heights, chunking, the ROWS tail
    for fwd in ("rows", "plain"):
        assert [t for t in box if t[3]["fwd"] == fwd], fwd
    for blocked in (False, True):
        assert [t for t in box if t[3]["fwd"] == "plain" and t[3]["blocked"] == blocked], blocked
    assert all(t[3]["blocked"] for t in lv if t[3]["fwd"] == "rows")
    assert {c["S"] for c in _rows(lay, entry="layout_pyramid", masks=None)} >= {8, 12, 20, 32, 40, 128, 512, 1024}
    for S in (8, 12, 20, 32, 40, 128, 512, 1024):
        assert [t for t in box if t[0]["S"] == S and t[2] == (t[0]["H"], t[0]["W"])], S
    assert {t[2][1] for t in box} >= {36, 40, 64, 320} and {t[2][0] for t in box} >= {2, 8, 31, 32, 34}
    assert [t for t in box if t[0]["S"] == 8 and t[2][1] == 320 and t[3]["chunks"] == 2 and 320 % t[3]["pxc"]]
    assert [t for t in box if t[3]["fwd"] == "rows" and t[3]["chunks"] >= 2 and t[2][1] % t[3]["pxc"]]
    assert [t for t in box if t[3]["fwd"] == "plain" and t[3]["chunks"] >= 2 and t[2][1] % t[3]["pxc"]]
    assert [t for t in box if t[3]["fwd"] == "rows" and t[2][0] % gc.LAY_ROWS]
    # an OW that is no multiple of 8 with S/4 dividing 256 leaves the blocked path even at OH >= 32
    assert [t for t in box if 256 % (t[0]["S"] // 4) == 0 and t[2][1] % 8 and t[2][0] >= 32 and t[3]["fwd"] == "plain" and
            not t[3]["blocked"]]
    # S/4 not dividing 256 on a map of 32 rows or more
    assert [t for t in box if 256 % (t[0]["S"] // 4) and t[2][0] >= 32 and t[3]["fwd"] == "plain"]
    # more dynamic LDS than the 64 KB a launch gets without asking
    assert [t for t in box if t[0]["S"] == 512 and t[3]["lds"] > 65536] and [t for t in box if t[0]["S"] == 1024 and t[3]["lds"] > 131072]
    assert all(t[3]["lds"] <= 160 * 1024 for t in lv)
    assert {(c["H"], c["W"]) for c in lay} >= {(24, 40), (64, 48)}
    assert [t for t in lv if t[2] != (t[0]["H"], t[0]["W"])]
    # ---- object counts
    assert {c["O"] for c in lay} >= {0, 1, 33, 300}
    assert _rows(lay, O=33, boxes="full") and _rows(lay, O=300, valid="gaps") and _rows(lay, valid="img1_none")
    for c in _rows(lay, O=33, boxes="full", masks=None):
        d = gc.make_data(c)
        for i, r in enumerate(gc.level_rules(c)):        # the second staging group of both forward kernels
            assert gc.tile_survivors(c, d, i, gc.LAY_ROWS if r["fwd"] == "rows" else 1) > gc.LAY_OB, c["name"]
    full = _levels(_rows(lay, O=33, boxes="full", masks=None))
    assert {(t[3]["fwd"], t[3]["blocked"]) for t in full} == {("rows", True), ("plain", True), ("plain", False)}
    big = _rows(lay, O=300)[0]
    assert big["O"] > gc.LAY_CULL and bool(gc.make_data(big)["valid"][:, gc.LAY_CULL:].any())
    # ---- backward to vecs: tiled, bd256, bd1024; > LAY_BB survivors; a pyramid that mixes them; npl = 1
    for bwd in ("tiled", "bd256", "bd1024"):
        assert [t for t in box if t[3]["bwd"] == bwd and "boxes" not in t[0]["need"]], bwd
    many = [(c, i) for (c, i, _, r) in box if r["bwd"] == "tiled" and gc.tile_survivors(c, gc.make_data(c), i, gc.LAY_ROWS) > gc.LAY_BB]
    assert many
    mix = [c for c in lay if len(c["sizes"]) >= 3 and {"tiled"} < {r["bwd"] for r in gc.level_rules(c)}]
    assert mix
    assert [t for t in lv if t[3]["npl"] == 1 and t[0]["S"] == 1024]
    assert [t for t in box if t[3]["bwd"] == "tiled" and t[3]["chunks"] >= 2 and t[2][0] % gc.LAY_ROWS]
    # ---- backward to boxes, without and with masks, on four families; both block sizes; accumulation with dboxes
    for masked in (False, True):
        for fam in ("inside", "border", "thin", "mixed"):
            assert [c for c in lay if "boxes" in c["need"] and c["boxes"] == fam and bool(c["masks"]) == masked and
                    c["entry"] == "layout_pyramid"], (masked, fam)
        for bwd in ("bd256", "bd1024"):
            assert [t for t in lv if "boxes" in t[0]["need"] and bool(t[0]["masks"]) == masked and t[3]["bwd"] == bwd], (masked, bwd)
    assert [c for c in lay if "boxes" in c["need"] and len(c["sizes"]) >= 2 and c["entry"] == "layout_pyramid"]
    assert all(r["bwd"] != "tiled" for c in lay if "boxes" in c["need"] or c["masks"] for r in gc.level_rules(c))
    for fam in gc.BOX_FAMILIES:
        assert _rows(lay, boxes=fam), fam
        assert [t for t in box if t[0]["boxes"] == fam and (t[3]["fwd"] == "rows" or fam in ("outside", "reversed"))], fam
    # ---- backward to masks: M, int / soft, accumulating (pyramid of >= 2 levels) and overwriting (disc_input)
    for entry in ("layout_pyramid", "disc_input"):
        got = [c for c in lay if c["entry"] == entry and "masks" in c["need"]]
        assert {c["masks"][1] for c in got} >= {1, 16, 32}, entry
        assert all(c["masks"][0] == "soft" for c in got)
    assert [c for c in lay if c["entry"] == "layout_pyramid" and "masks" in c["need"] and len(c["sizes"]) >= 2]
    for kind in ("int", "soft"):
        assert [c for c in lay if c["masks"] and c["masks"][0] == kind and c["H"] != c["W"] and len(c["sizes"]) >= 2], kind
        for M in (1, 16, 32):
            assert [c for c in LAYOUT if c["masks"] == (kind, M)], (kind, M)
    # ---- disc_input
    di = _rows(lay, entry="disc_input")
    assert {c["S"] for c in di} >= {8, 12, 32, 128} and {c["img_fmt"] for c in di} == {"nchw", "cl"}
    assert [c for c in di if c["masks"]] and [c for c in di if not c["masks"]]
    assert {r["fwd"] for c in di for r in gc.level_rules(c)} == {"rows", "plain"}
    # ---- the ABI's channel slice
    ab = _rows(lay, entry="abi_slice")
    assert {c["out_off"] for c in ab} >= {4, 36} and all(c["out_cs"] > c["S"] + c["out_off"] for c in ab)
    assert {r["fwd"] for c in ab for r in gc.level_rules(c)} == {"rows", "plain"}
    assert {r["bwd"] for c in ab for r in gc.level_rules(c)} >= {"tiled", "bd256", "bd1024"}
    assert [c for c in ab if "boxes" in c["need"]] and [c for c in ab if c["masks"]]
    # ---- paint
    pt = _rows(LAYOUT, entry="layout_paint")
    assert {c["masks"] for c in pt} >= {(k, M) for k in ("int", "soft") for M in (1,)} | {("int", 16), ("soft", 32), ("int", 32)}
    assert {c["masks"][1] for c in pt} >= {1, 16, 32} and {c["masks"][0] for c in pt} == {"int", "soft"}
    assert [c for c in pt if c["H"] != c["W"]] and [c for c in pt if c["H"] == c["W"]]
    assert all(len(c["sizes"]) >= 2 and c["sizes"][1] != (c["H"], c["W"]) for c in pt)
    assert len({(c["B"], c["H"], c["W"]) for c in pt}) >= 3 and [c for c in pt if c["valid"] == "ragged"]
    # ---- crops
    cr = _rows(RUN, family="crop")
    grad = [c for c in cr if "img" in c["need"]]
    assert {c["C"] for c in grad} >= {1, 3, 4} and {(c["H"], c["W"]) for c in grad} >= {(64, 64), (40, 72), (17, 129)}
    assert {c["HH"] for c in grad} >= {1, 8, 32, 64} and {c["N"] for c in grad} >= {0, 1, 300}
    assert _rows(grad, N=300, B=2) and gc.CROP_MAXHW == 64
    assert [c for c in grad if gc.crop_tile_candidates(c, gc.make_data(c)) > gc.CROP_K]
    assert [c for c in grad if c["boxes"] == "full" and gc.crop_tile_candidates(c, gc.make_data(c)) > gc.CROP_K]
    un = _rows(grad, idx="unsorted")
    assert un
    for c in un:
        idx = gc.make_data(c)["img_idx"]
        assert bool((idx[1:] < idx[:-1]).any()) and 1 not in idx.tolist() and c["B"] >= 3
    for fam in gc.BOX_FAMILIES:
        assert _rows(grad, boxes=fam), fam
        assert [c for c in grad if c["boxes"] == fam and ("boxes" in c["need"])], fam
    thin = _rows(grad, boxes="thin")[0]
    s = gc.crop_slopes(thin, gc.make_data(thin))
    assert bool((s.abs() < 1e-3).any(1).all())                       # every crop of the row scans everything on an axis
    small = [c for c in grad if c["HH"] == 64 and float(gc.crop_slopes(c, gc.make_data(c)).min()) < 0.5]
    assert small                                                      # slopes well below one pixel: the widest windows
    fwd_only = [c for c in cr if not c["need"]]
    assert [c for c in fwd_only if c["C"] == 8] and [c for c in fwd_only if c["HH"] == 96]
    ref = _rows(CASES, refuse=lambda r: r is not None)
    for c in fwd_only:
        assert [r for r in ref if (r["C"], r["HH"], r["H"], r["N"]) == (c["C"], c["HH"], c["H"], c["N"]) and r["need"]], c["name"]
    # ---- nothing near 2^31 elements
    for c in CASES:
        sides = [c["B"] * c["C"] * c["H"] * c["W"], c["N"] * 8 * c["HH"] ** 2] if c["family"] == "crop" else \
                [c["B"] * (c["out_cs"] or c["S"] + 4) * h * w for (h, w) in c["sizes"]] + [c["B"] * c["O"] * c["S"]]
        assert max(sides) < 2 ** 27, c["name"]


def test_tiled_rule_matches_the_library():
    """The restated layout_bwd_tiled against csg_layout_bwd_workspace (the library loads without a device)."""
    from canonicalsg2im_amd import _lib
    for c in LAYOUT:
        for (h, w), r in zip(c["sizes"], gc.level_rules(c)):
            for has_masks in (0, 1):
                for dboxes in (0, 1):
                    rule = gc.level_rule(c["S"], h, w, c["O"], ("soft", 16) if has_masks else None, bool(dboxes))
                    nws = _lib.lib.csg_layout_bwd_workspace(c["B"], c["O"], c["S"], h, w, has_masks, dboxes)
                    want = 0
                    if rule["bwd"] == "tiled":
                        n = c["B"] * rule["ntiles"] * c["O"]
                        want = n * c["S"] * 4 + (n + 15) // 16 * 16
                    assert nws == want, (c["name"], (h, w), has_masks, dboxes, nws, want)
