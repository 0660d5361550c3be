"""The direct-convolution matrix on the CPU (tests/igemm_cases.py): the restated launch rules against the library's own
workspace queries (the library loads without a device; nothing is launched); the table's coverage of every launch class,
with each rule's boundary present on both sides; the Inception census; `desc_ref64` / `wgrad_ref64` against torch's own
float64 convolutions; and, for every row, that the buffers the device test allocates contain every address the descriptor
can produce."""
import inspect
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import igemm_cases as ic
from igemm_cases import CASES, ENTRY_CASES, case_ids, desc_array as _desc_array, to_ctypes

RUN = [c for c in CASES if not c["refuse"]]
FWD = [c for c in RUN if c["kind"] == "fwd"]
MULTI = [c for c in RUN if c["kind"] == "multi"]
WGRAD = [c for c in RUN if c["kind"] == "wgrad"]


def _one(name):
    (c,) = [c for c in CASES if c["name"] == name]
    return c


# ------------------------------------------------------------------------------------------------ the rules against the library
def _sweep():
    """~400 forward descriptors on and around every rule's boundary: tiles 1 .. 4200, K tiles 1 .. 72, every block width."""
    out = []
    for (B, H, W), (cin, k), cout in itertools.product(
            ((1, 1, 1), (2, 3, 3), (2, 9, 9), (1, 82, 100), (2, 82, 100), (4, 129, 129), (120, 17, 17), (4, 128, 128), (50, 35, 35),
             (9, 130, 130), (8, 256, 256)),
            ((8, 1), (64, 3), (480, 1), (512, 1), (544, 1), (192, 7)), (6, 8, 32, 64, 192, 1024)):
        out.append(ic.conv_desc(B, H, W, cin, cout, 1 if k == 7 else k, k))
    return out


def test_restated_rules_match_the_library():
    from canonicalsg2im_amd._lib import lib
    seen = set()
    for d in _sweep() + [d for c in FWD for d in c["descs"]] + [d for e in ENTRY_CASES for d in ic.entry_descs(e)]:
        want = ic.fwd_workspace_bytes(d)
        assert lib.csg_conv_fwd_workspace(to_ctypes(d)) == want, (d, want)
        seen.add(ic.fwd_class(d)[1])
    assert seen == {"plain", "split", "tail"}
    for c in MULTI:
        plans, floats = ic.multi_plan(c["descs"])
        assert lib.csg_conv_fwd_multi_workspace(_desc_array(c["descs"]), len(c["descs"])) == 4 * floats, c["name"]
    for d in _sweep() + [c["descs"][0] for c in WGRAD]:
        if d["Cout"] % 4 == 0:
            assert lib.csg_conv_bwd_weight_workspace(to_ctypes(d)) == ic.wgrad_workspace_bytes(d), d


def test_library_refuses_what_the_refusal_rows_say_it_checks_first():
    """The two multi refusals are decided by the workspace query already (no device needed): -1."""
    from canonicalsg2im_amd._lib import last_error, lib
    for name in ("refuse_multi_five", "refuse_multi_channels"):
        c = _one(name)
        assert lib.csg_conv_fwd_multi_workspace(_desc_array(c["descs"]), len(c["descs"])) == -1, name
        assert re.search(c["refuse"], last_error()), (name, last_error())


# ------------------------------------------------------------------------------------------------ coverage
FWD_CLASSES = {
    # block width, whole launches, vector epilogue: write | accumulate
    (32, "plain", "set", "vec"), (64, "plain", "set", "vec"), (128, "plain", "set", "vec"),
    (32, "plain", "acc", "vec"), (64, "plain", "acc", "vec"), (128, "plain", "acc", "vec"),
    # the scalar epilogue
    (32, "plain", "set", "scalar"), (32, "plain", "acc", "scalar"),
    # uniform split-K (k_splitk_epilogue): write | accumulate, the three widths, and a y_cs the vector stores cannot take
    (32, "split", "set", "vec"), (64, "split", "set", "vec"), (64, "split", "acc", "vec"), (128, "split", "set", "vec"), (32, "split", "acc", "scalar"),
    # the tail split
    (128, "tail", "set", "vec"), (128, "tail", "acc", "vec"), (32, "tail", "set", "vec"), (64, "tail", "set", "vec"),
    (128, "tail", "acc", "scalar"),
}
WGRAD_CLASSES = {(bi, j, "one", db) for bi in (32, 64, 128) for j in ("j1",) for db in ("db", "nodb")} | {
    (32, "j>1", "one", "nodb"), (32, "j>1", "split", "db"), (32, "j>1", "split", "nodb"), (128, "j>1", "split", "db"),
    (128, "j>1", "split", "nodb")}


def test_table_names_every_launch_class():
    names = case_ids()
    assert len(set(names)) == len(names)
    for c in RUN:                                                      # `cls` is what the rules give, not what was typed
        if c["kind"] == "wgrad":
            assert c["cls"] == (ic.wgrad_class(c["descs"][0], c["db"]),), c["name"]
        elif c["kind"] == "fwd":
            assert c["cls"] == tuple(ic.fwd_class(d) for d in c["descs"]), c["name"]
    have = {k for c in FWD for k in c["cls"]}
    assert FWD_CLASSES <= have, sorted(FWD_CLASSES - have)
    have = {k for c in WGRAD for k in c["cls"]}
    assert WGRAD_CLASSES <= have, sorted(WGRAD_CLASSES - have)
    # multi: a launch that splits (ws_off differs per class) and one that does not; odd maps (class sizes differ) and even
    split = {(any(p["ksplit"] > 1 for p in ic.multi_plan(c["descs"])[0]), len({d["OHg"] * d["OWg"] for d in c["descs"]}) > 1) for c in MULTI}
    assert split == {(True, True), (True, False), (False, True), (False, False)}
    assert {(split_, c["bias"] and c["res"]) for c in MULTI for split_ in [ic.multi_plan(c["descs"])[1] > 0]} >= {
        (False, False), (False, True), (True, False), (True, True)}       # bias and residual in both epilogues of the multi launch
    for c in MULTI:
        plans, floats = ic.multi_plan(c["descs"])
        assert len(c["descs"]) == 4 and len({tuple(d["tap_w"]) for d in c["descs"]}) == 4
        if floats:
            assert len({p["ws_off"] for p in plans}) == 4, c["name"]
    # every refusal the issue lists
    assert {c["name"] for c in CASES if c["refuse"]} == {
        "refuse_short_workspace", "refuse_gate_act", "refuse_gate_acc", "refuse_multi_five", "refuse_multi_channels",
        "refuse_wg_partial_taps"}


def test_every_rule_boundary_is_present_on_both_sides():
    """Typed-in expectations: a changed constant in the restated rules, or a row whose shape drifted, fails here."""
    plan = {c["name"]: ic.fwd_plan(c["descs"][0]) for c in FWD}
    want_bn = {4: 32, 20: 32, 32: 32, 36: 64, 64: 64, 68: 128, 128: 128, 132: 128, 192: 128, 320: 128}
    for cout, bn in want_bn.items():
        p = plan["cout%d" % cout]
        assert (p["bn"], p["ntiles"]) == (bn, ic.cdiv(cout, bn)), cout
    assert [(plan["m%d" % m]["M"], plan["m%d" % m]["mtiles"]) for m in (1, 127, 128, 129)] == [(1, 1), (127, 1), (128, 1), (129, 2)]
    assert plan["map1x1_b300"]["M"] == 300 and _one("map1x1_b300")["descs"][0]["OHg"] == 1
    assert [_one("ow%d" % w)["descs"][0]["OWg"] for w in (1, 3, 7, 257)] == [1, 3, 7, 257]
    assert [plan["nkt%d" % k]["nkt"] for k in range(1, 8)] == list(range(1, 8))
    assert [_one("cin%d" % c)["descs"][0]["Cin"] for c in (4, 8, 12, 20, 36, 48)] == [4, 8, 12, 20, 36, 48]
    assert 32 % 12 and 32 % 20 and plan["ktot100"]["Ktot"] == 100
    # uniform split: 15 | 16 K tiles; a short last split; four splits of a one-tile-row grid; Cout % 4 != 0 never splits
    assert (plan["nkt15_plain"]["nkt"], plan["nkt15_plain"]["ksplit"]) == (15, 1)
    assert (plan["nkt16_split"]["nkt"], plan["nkt16_split"]["ksplit"], plan["nkt16_split"]["kt_per"]) == (16, 2, 8)
    assert (plan["nkt17_short_last"]["nkt"], plan["nkt17_short_last"]["ksplit"], plan["nkt17_short_last"]["kt_per"]) == (17, 2, 9)
    assert (plan["ksplit4_m2"]["M"], plan["ksplit4_m2"]["ntiles"], plan["ksplit4_m2"]["nkt"], plan["ksplit4_m2"]["ksplit"]) == (2, 3, 36, 4)
    assert (plan["cout6_k512_plain"]["nkt"], plan["cout6_k512_plain"]["ksplit"]) == (16, 1)
    p = plan["split_acc_5x5"]
    assert (p["Ktot"], p["nkt"], p["ksplit"]) == (9 * 64, 18, 2) and _one("split_acc_5x5")["descs"][0]["tap_w"] == list(range(16, 25))
    for name in ("split_res", "split_gate", "split_y_slice", "split_scalar_cs6", "split_bn64", "split_bn128"):
        assert plan[name]["ksplit"] == 2 and plan[name]["tail"] is None, name
    # the tail split: (tiles, first split tile, slabs, first slab row)
    want = {"tail_nt8": (65 * 8, 512, 2, 8192), "tail_nt4": (129 * 4, 512, 2, 16384), "tail_nt1_bn32": (521, 512, 2, 65536),
            "tail_nt2_5slabs": (271 * 2, 512, 5, 32768), "tail_acc": (520, 512, 2, 8192), "tail_res": (520, 512, 2, 8192),
            "tail_y_slice": (520, 512, 2, 8192), "tail_bn64": (516, 512, 2, 65536), "tail_scalar_cs1030_acc": (520, 512, 2, 8192)}
    for name, (tiles, tile0, ks, m0) in want.items():
        p = plan[name]
        assert p["tail"] is not None and p["ksplit"] == 1, name
        assert (p["mtiles"] * p["ntiles"], p["tail"]["tile0"], p["tail"]["ks"], p["tail"]["m0"]) == (tiles, tile0, ks, m0), name
        assert p["M"] > m0 and p["tail"]["ks"] * p["tail"]["kt_per"] >= p["nkt"] > (p["tail"]["ks"] - 1) * p["tail"]["kt_per"], name
    assert plan["tail_nt1_bn32"]["bn"] == 32 and plan["tail_nt2_5slabs"]["M"] == 120 * 17 * 17
    p = plan["m65536_nt1_plain"]
    assert (p["M"], p["mtiles"] * p["ntiles"], p["ksplit"], p["tail"]) == (65536, 512, 1, None) and p["nkt"] >= 16
    # partial tap lists of one 5x5 weight, slices, the folded upsample
    assert _one("taps5x5_first0")["descs"][0]["tap_w"] == list(range(16)) and _one("taps5x5_first16")["descs"][0]["tap_w"] == list(range(16, 25))
    assert all(_one(n)["descs"][0]["wtaps"] == 25 for n in ("taps5x5_first0", "taps5x5_first16", "split_acc_5x5"))
    d = _one("up1_even")["descs"][0]
    assert (d["in_up"], d["IHv"], d["IWv"]) == (1, 2 * d["IHp"], 2 * d["IWp"])
    d = _one("up1_odd")["descs"][0]
    assert (d["in_up"], d["IHv"], d["IWv"]) == (1, 2 * d["IHp"] - 1, 2 * d["IWp"] - 1)
    assert _one("x_slice")["descs"][0]["x_cs"] == 8 + 8 and (_one("y_slice")["descs"][0]["y_cs"], _one("y_slice")["y_off"]) == (8 + 12, 4)
    # weight gradient: tile heights, 128 | 132 columns, the pixel counts, 1 .. 7 chunks per split, the library's two splits
    wp = {c["name"]: ic.wgrad_plan(c["descs"][0]) for c in WGRAD}
    assert [(wp["wg_cout%d" % c]["bi"], wp["wg_cout%d" % c]["itiles"]) for c in (32, 36, 64, 68, 128, 160)] == [
        (32, 1), (64, 1), (64, 1), (128, 1), (128, 1), (128, 2)]
    assert (wp["wg_ktot128"]["jtiles"], wp["wg_ktot132"]["jtiles"]) == (1, 2)
    assert [(wp["wg_m%d" % m]["M"], wp["wg_m%d" % m]["nch"]) for m in (31, 32, 33, 255, 257)] == [(31, 1), (32, 1), (33, 2), (255, 8), (257, 9)]
    chunks = {n for c in WGRAD for n in ic.chunks_per_split(c["descs"][0])}
    assert chunks >= set(range(1, 10)), sorted(chunks)
    assert [ic.chunks_per_split(_one("wg_chunks%d" % k)["descs"][0]) for k in range(3, 8)] == [[k] for k in range(3, 8)]
    assert (wp["wg_split12"]["nsplit"], wp["wg_split12"]["cps"], wp["wg_split12_db"]["nsplit"]) == (12, 9, 12)
    assert (wp["wg_split3"]["nsplit"], wp["wg_split3_db"]["nsplit"], wp["wg_split3"]["M"]) == (3, 3, 3 * 16 * 16)
    assert wp["wg_66564_terms"]["M"] == 66564
    assert (_one("wg_y_slice")["descs"][0]["y_cs"], _one("wg_x_slice")["descs"][0]["x_cs"]) == (44, 16)
    assert _one("wg_up1_odd")["descs"][0]["IHv"] == 7 and _one("refuse_wg_partial_taps")["descs"][0]["ntaps"] == 16
    # the entry rows: the second launch of the 5x5 layer splits and accumulates; the (1,7) layer at batch 120 tail-splits
    a, b = ic.entry_descs(ENTRY_CASES[0])
    assert (ic.fwd_class(a)[:3], ic.fwd_class(b)[:3]) == ((64, "split", "set"), (64, "split", "acc"))
    (t,) = ic.entry_descs(ENTRY_CASES[1])
    assert ic.fwd_class(t) == (128, "tail", "set", "vec") and ic.fwd_plan(t)["tail"]["ks"] == 5


def test_inception_census_falls_into_classes_the_table_has():
    """Every Inception-v3 layer that reaches ops.conv2d_forward, at its real map (35 / 17 / 8) and batch 1, 2 and 50: six
    launch classes, none of them the tail split - which batch 120 does reach (Mixed_7a.branch7x7x3_3)."""
    from canonicalsg2im_amd import inception
    layers, blocks = [tuple(L) for L in inception.layer_table()], inception.BLOCKS
    cen = ic.census(layers, blocks)
    # A: 4 branch ends x 3 blocks; B: 2; C: 4 ends + 4 rectangular x 4; D: 2 + 2; E: 6 x 2 - 62 layers, the three 5x5 ones twice
    assert len(cen) == 3 * 62 and sum(len(v) for v in cen.values()) == 3 * 65
    classes = {k for v in cen.values() for k in v}
    assert classes == {(32, "plain", "set", "vec"), (64, "plain", "set", "vec"), (64, "plain", "acc", "vec"),
                       (64, "split", "set", "vec"), (128, "split", "set", "vec"), (128, "plain", "set", "vec")}
    have = {k for c in FWD for k in c["cls"]}
    assert classes <= have, sorted(classes - have)
    big = ic.census(layers, blocks, batches=(120,))
    assert big[("Mixed_7a.branch7x7x3_3", 120)] == [(128, "tail", "set", "vec")] and (128, "tail", "set", "vec") in have


# ------------------------------------------------------------------------------------------------ the reference against torch
def _nchw(t, off, n):
    return t[..., off:off + n].permute(0, 3, 1, 2).double()


def _close(name, got, ref):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert scale > 0 and err <= 1e-12 * scale, "%s: %.3e of scale %.3e" % (name, err, scale)


def _virtual_input(d, x, x_off):
    xv = _nchw(x, x_off, d["Cin"])
    if d["in_up"]:
        xv = F.interpolate(xv, scale_factor=2 ** d["in_up"], mode="nearest")
    return xv[:, :, :d["IHv"], :d["IWv"]]


@pytest.mark.parametrize("c", FWD, ids=case_ids(FWD))
def test_desc_ref64_is_torchs_convolution(c):
    (d,), g, data = c["descs"], c["conv"], ic.make_data(c)
    got, own = ic.desc_ref64(d, data["x"], data["w"], data["bias"], data["res"], data["y0"], c["x_off"], c["y_off"])
    w = data["w"].double().clone()
    listed = torch.zeros(d["wtaps"], dtype=torch.bool)
    listed[d["tap_w"]] = True
    w[:, ~listed] = 0                                                  # a partial tap list: the other taps do not take part
    w = w.view(g["Cout"], g["KH"], g["KW"], g["Cin"]).permute(0, 3, 1, 2)
    v = F.conv2d(_virtual_input(d, data["x"], c["x_off"]), w, None if data["bias"] is None else data["bias"].double(), g["stride"], g["pad"])
    slope = float(torch.tensor(d["slope"], dtype=torch.float32))
    if d["act"] == ic.ACT_LEAKY:
        v = F.leaky_relu(v, slope)
    elif d["act"] == ic.ACT_TANH:
        v = torch.tanh(v)
    if data["res"] is not None:
        r = _nchw(data["res"], c["y_off"], d["Cout"])
        v = v * ((r > 0).double() + (r <= 0).double() * slope) if d["res_gate"] else v + r
    if d["accumulate"]:
        v = v + _nchw(data["y0"], c["y_off"], d["Cout"])
    _close(c["name"], _nchw(got, c["y_off"], d["Cout"]), v)
    rest = got.clone()
    rest[..., c["y_off"]:c["y_off"] + d["Cout"]] = data["y0"].double()[..., c["y_off"]:c["y_off"] + d["Cout"]]
    assert torch.equal(rest, data["y0"].double()) and int(own.sum()) == v.numel(), c["name"]   # nothing beside the slice moved
    if d["res_gate"]:
        r = data["res"][..., c["y_off"]:c["y_off"] + d["Cout"]]
        assert bool((r == 0).any()) and bool((r > 0).any()) and bool((r < 0).any()), c["name"]


@pytest.mark.parametrize("c", MULTI, ids=case_ids(MULTI))
def test_class_descriptors_are_the_transposed_convolution(c):
    g, data = c["conv"], ic.make_data(c)
    got = ic.reference(c, data)
    assert bool(got["own"].all()), c["name"]                           # the four classes tile dX: no sentinel survives
    dy = data["x"].permute(0, 3, 1, 2).double()
    w = data["w"].double().view(g["Cin"], 4, 4, g["Cout"]).permute(3, 0, 1, 2)           # packed [Cin][ky][kx][Cout]
    extra = 0.0
    if c["bias"]:
        extra = extra + data["bias"].double().view(1, -1, 1, 1)
    if c["res"]:
        extra = extra + data["res"].permute(0, 3, 1, 2).double()
    want = torch.nn.grad.conv2d_input((g["B"], g["Cin"], g["IH"], g["IW"]), w, dy, g["stride"], g["pad"])
    _close(c["name"], got["y"].permute(0, 3, 1, 2), want + extra)
    _close(c["name"] + " (conv_transpose2d)", got["y"].permute(0, 3, 1, 2), extra + F.conv_transpose2d(
        dy, w, None, g["stride"], g["pad"], output_padding=(g["IH"] % 2, g["IW"] % 2)))


@pytest.mark.parametrize("c", WGRAD, ids=case_ids(WGRAD))
def test_wgrad_ref64_is_torchs_weight_gradient(c):
    (d,), g, data = c["descs"], c["conv"], ic.make_data(c)
    got = ic.reference(c, data)
    dy = _nchw(data["dy"], c["y_off"], d["Cout"])
    want = torch.nn.grad.conv2d_weight(_virtual_input(d, data["x"], c["x_off"]), (g["Cout"], g["Cin"], g["KH"], g["KW"]), dy, g["stride"], g["pad"])
    _close(c["name"] + " dw", got["dw"], want.permute(0, 2, 3, 1).reshape(d["Cout"], d["wtaps"], d["Cin"]))
    if c["db"]:
        _close(c["name"] + " db", got["db"], dy.sum((0, 2, 3)))
    else:
        assert got["db"] is None


def test_entry_rows_are_torchs_convolution():
    """The launches conv2d_forward makes, applied in order by desc_ref64, then bias and ReLU on the sum: F.conv2d."""
    e = ENTRY_CASES[0]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(e["B"], e["H"], e["W"], e["Cin"], generator=g)
    w = torch.randn(e["Cout"], e["KH"] * e["KW"], e["Cin"], generator=g) / 40
    y = torch.full((e["B"], e["H"], e["W"], e["wide"]), ic.SENTINEL)
    for d in ic.entry_descs(e):
        y, _ = ic.desc_ref64(d, x, w, None, None, y, 0, e["off"])
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double().view(e["Cout"], e["KH"], e["KW"], e["Cin"]).permute(0, 3, 1, 2), None, 1, e["pad"])
    _close(e["name"], _nchw(y, e["off"], e["Cout"]), want)


# ------------------------------------------------------------------------------------------------ addresses
def _input_extent(d):
    """(largest physical row, largest physical column) any tap of any grid point reads, or None when every tap is outside."""
    best = None
    for t in range(d["ntaps"]):
        iy = torch.arange(d["OHg"]) * d["istride"] + d["tap_dy"][t]
        ix = torch.arange(d["OWg"]) * d["istride"] + d["tap_dx"][t]
        iy, ix = iy[(iy >= 0) & (iy < d["IHv"])], ix[(ix >= 0) & (ix < d["IWv"])]
        if iy.numel() and ix.numel():
            e = (int(iy.max()) >> d["in_up"], int(ix.max()) >> d["in_up"])
            best = e if best is None else (max(best[0], e[0]), max(best[1], e[1]))
    return best


@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_every_address_lies_inside_the_rows_buffers(c):
    """The largest output pixel * y_cs + Cout, the largest input pixel * x_cs + Cin and the weights Cout * wtaps * Cin, from
    the descriptor alone, against what the device test allocates (igemm_cases.buffers)."""
    shapes = ic.buffers(c)
    numel = {k: int(torch.Size(s).numel()) for k, s in shapes.items()}
    out = "dy" if "dy" in shapes else "y"
    for d in c["descs"][:4]:
        if c["name"] == "refuse_multi_channels" and d["Cout"] != c["descs"][0]["Cout"]:
            continue                                                   # refused before anything is addressed
        assert d["Cin"] % 4 == 0 and d["x_cs"] % 4 == 0 and c["x_off"] % 4 == 0 and c["x_off"] + d["Cin"] <= d["x_cs"], c["name"]
        assert c["y_off"] + d["Cout"] <= d["y_cs"] and 1 <= d["ntaps"] <= ic.MAX_TAPS, c["name"]
        ext = _input_extent(d)
        assert ext is not None and ext[0] < d["IHp"] and ext[1] < d["IWp"], c["name"]
        last_in = ((d["B"] - 1) * d["IHp"] + ext[0]) * d["IWp"] + ext[1]
        assert last_in * d["x_cs"] + c["x_off"] + d["Cin"] <= numel["x"], c["name"]
        oy, ox = (d["OHg"] - 1) * d["os"] + d["ooy"], (d["OWg"] - 1) * d["os"] + d["oox"]
        assert oy < d["OHf"] and ox < d["OWf"], c["name"]
        last_out = ((d["B"] - 1) * d["OHf"] + oy) * d["OWf"] + ox
        assert last_out * d["y_cs"] + c["y_off"] + d["Cout"] <= numel[out], c["name"]
        assert max(d["tap_w"]) < d["wtaps"] and min(d["tap_w"]) >= 0 and d["Cout"] * d["wtaps"] * d["Cin"] == numel["w"], c["name"]
        assert numel["x"] * 4 < 2 ** 31 and numel[out] * 4 < 2 ** 31                      # 32-bit buffer offsets with room
        if out == "dy":
            assert numel["dw"] == numel["w"] and numel["db"] == d["Cout"] and d["Cout"] % 4 == 0 and d["y_cs"] % 4 == 0
            assert c["y_off"] % 4 == 0
        elif (d["Cout"] | d["y_cs"]) & 3 == 0:
            assert c["y_off"] % 4 == 0, c["name"]                      # the vector epilogue stores 16 bytes at a time
    for e in ENTRY_CASES:
        assert e["off"] % 4 == 0 and e["wide"] % 4 == 0 and e["off"] + e["Cout"] < e["wide"], e["name"]


def test_no_reads_from_outside_the_repository():
    for mod in (ic, __import__("test_gpu_igemm_paths")):
        src = inspect.getsource(mod)
        assert not re.search(r"""["'](/|~|\.\./)[A-Za-z_.]""", src), mod.__name__
        assert set(re.findall(r"environ[^\n]*?[\"']([A-Z_]+)[\"']", src)) <= {"IGEMM_PATHS_REPORT"}, mod.__name__
    assert os.path.dirname(os.path.abspath(ic.__file__)) == os.path.dirname(os.path.abspath(__file__))
