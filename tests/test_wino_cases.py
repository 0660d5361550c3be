"""The Winograd matrix on the CPU (tests/wino_cases.py): the table's coverage of every launch class; the restated launch
rules against the library's own workspace and pack-size queries (the library loads without a device; nothing is launched),
on every row and on a sweep around each rule's boundary; `wino_ref64` / `wino_wgrad_ref64` against torch's own float64
convolutions and autograd; a strided row against its dense twin on the same owned data; and every refusal that returns
before a device is touched, through the real entry points."""
import ctypes
import itertools
import re

import pytest
import torch
import torch.nn.functional as F

import wino_cases as wc
from wino_cases import CASES, case_ids, to_ctypes

RUN = [c for c in CASES if not c["refuse"]]
CONV = [c for c in RUN if c["entry"] != "wgrad"]
WGRAD = [c for c in RUN if c["entry"] == "wgrad"]
REFUSE = [c for c in CASES if c["refuse"]]
SMALL = [c for c in RUN if c["d"]["B"] * c["d"]["H"] * c["d"]["W"] * c["d"]["Cin"] * c["d"]["Cout"] <= 1 << 24]


def _one(name):
    (c,) = [c for c in CASES if c["name"] == name]
    return c


# ------------------------------------------------------------------------------------------------ coverage
def test_table_reaches_every_launch_class():
    names = case_ids()
    assert len(set(names)) == len(names)
    for c in RUN:                                                      # `cls` is what the rules give, not what was typed
        assert c["cls"] == wc.classify(c), c["name"]
    have = set().union(*[c["cls"] for c in RUN])
    want = wc.all_classes()
    assert want <= have, "classes no row reaches: %s" % sorted(map(str, want - have))
    assert have <= want, "classes the rules do not enumerate: %s" % sorted(map(str, have - want))


def test_every_rule_boundary_is_where_the_issue_puts_it():
    """Typed-in expectations: a changed constant in the restated rules, or a row whose shape drifted, fails here."""
    plan = {c["name"]: wc.run_plan(c) for c in CONV if c["entry"] != "spade"}
    assert [(plan[n][0]["ksplit"], plan[n][0]["sps"], plan[n][1]) for n in
            ("f2_stages15_plain", "f2_split_min", "f2_split_uneven17", "f2_split_ksplit_below_ks")] == [
        (1, 15, "plain"), (2, 8, "split"), (2, 9, "split"), (9, 9, "split")]
    assert plan["f2_split_ksplit_below_ks"][0]["first_ks"] == 10
    assert [(plan[n][0]["ksplit"], plan[n][0]["sps"]) for n in ("f4_split_min", "f4_split_c100", "f34_split_min")] == [(2, 16), (2, 17), (2, 16)]
    for n in ("f2_split_strided_y_runs_unsplit", "f4_split_strided_y_runs_unsplit"):
        c = _one(n)
        assert plan[n][1] == "unsplit-strided-y" and wc.conv_workspace_bytes(c["fam"], c["d"]) == 0
        assert wc.conv_workspace_bytes(c["fam"], dict(c["d"], y_cs=c["d"]["Cout"])) > 0
    assert {(wc.wn_plan(c["d"])["TW"], wc.wn_plan(c["d"])["ntb"]) for c in CONV if c["fam"] == "f2"} == {
        (tw, n) for tw in (4, 8, 16) for n in (1, 2)}
    # the persistent form: 512 items on 256 CUs and not one fewer; an odd stage count or Cout % 64 keeps the one-item form
    p = wc.w4_plan(_one("f4_persist_dense")["d"], 4)
    assert wc.w4_persistent_blocks(p, 512) == 256 and wc.w4_persistent_blocks(p, 511) == 0
    assert wc.w4_persistent_blocks(p, 512, cus=304) == 0 and wc.w4_persistent_blocks(p, 608, cus=304) == 304
    assert wc.w4_persistent_blocks(dict(p, nstage=3), 512) == 0 and wc.w4_persistent_blocks(dict(p, nstage=2), 512) == 0
    assert wc.w4_persistent_blocks(dict(p, Cout=480), 512) == 0 and wc.w4_persistent_blocks(dict(p, ksplit=2), 512) == 0
    for c in CONV:
        if c["both_forms"]:
            assert ("f4", "form", "persistent") in c["cls"], c["name"]
    # weight gradients: 8 regions stay one slice, 9 make two (F(3x3,2x2)); 16 and 17 (F(3x3,4x4))
    for fam, lo in (("wg2", 8), ("wg4", 16)):
        assert wc.wg_plan(fam, wc.wino_desc(lo, 8, 8, 64, 64))["nsplit"] == 1
        p = wc.wg_plan(fam, wc.wino_desc(lo + 1, 8, 8, 64, 64))
        assert (p["nsplit"], p["rps"]) == (2, (lo + 2) // 2)
    assert {wc.wn_wg_plan(c["d"])["tsx"] for c in WGRAD if c["fam"] == "wg2"} == {4, 8, 16}
    # the pad-2 1x1 map is admitted; a 4x4 filter with pad 1 on a 1x1 map is not
    assert isinstance(wc.w4_plan(wc.wino_desc(1, 1, 1, 8, 4), 3, 2), dict) and wc.w4_plan(wc.wino_desc(1, 1, 1, 8, 4), 3, 1) == wc.E_UNSUPPORTED
    assert {c["name"] for c in REFUSE} == {
        "refuse_f2_strided_x", "refuse_f4_strided_x", "refuse_f34_strided_x", "refuse_f4_part_strided_x", "refuse_f4_spade_strided_x",
        "refuse_f2_xcs_below_cin", "refuse_f4_xcs_mod4", "refuse_f34_ycs_below_cout", "refuse_f2_cin24", "refuse_f4_cin12",
        "refuse_f2_misaligned_x", "refuse_f4_misaligned_y", "refuse_f34_misaligned_packed", "refuse_f2_pack_misaligned",
        "refuse_f4_pack_misaligned", "refuse_wg2_short_workspace", "refuse_wg2_direct_short_workspace",
        "refuse_wg4_short_workspace", "refuse_f4_part_tiles", "refuse_f4_spade_unqualified"}
    # slices are 16-byte aligned and inside their buffers
    for c in RUN:
        d = c["d"]
        assert c["x_off"] % 4 == 0 and c["y_off"] % 4 == 0 and c["x_off"] + d["Cin"] <= d["x_cs"] and c["y_off"] + d["Cout"] <= d["y_cs"], c["name"]
        assert (c["x_off"] > 0) == (d["x_cs"] != d["Cin"]) and (c["y_off"] > 0) == (d["y_cs"] != d["Cout"]), c["name"]
        for key in ("part", "spade"):
            if c[key] and c[key].get("gamma_cs"):
                assert c[key]["g_off"] % 4 == 0 and c[key]["g_off"] + d["Cout"] <= c[key]["gamma_cs"] and c[key]["gamma_cs"] > d["Cout"], c["name"]


# ------------------------------------------------------------------------------------------------ the rules against the library
def _sweep():
    """Descriptors on and around every rule's boundary, dense and strided, served and refused."""
    out = []
    for (B, H, W), cin, cout, (xs, ys) in itertools.product(
            ((1, 2, 8), (1, 16, 32), (2, 20, 36), (1, 8, 8), (9, 8, 8), (17, 8, 8), (3, 4, 16), (9, 2, 32), (1, 6, 10), (1, 1, 1),
             (2, 2, 2), (1, 15, 15), (4, 64, 128), (6, 64, 128), (1, 128, 128), (16, 16, 16), (33, 32, 32), (1, 5, 9), (2, 3, 8)),
            (8, 16, 24, 32, 64, 128, 240, 256, 264, 272, 512, 1296, 12, 6), (4, 32, 36, 64, 100, 512, 6), ((0, 0), (8, 0), (0, 8), (8, 12), (2, 0), (-4, 0))):
        out.append(wc.wino_desc(B, H, W, cin, cout, cin + xs, cout + ys))
    out += [wc.wino_desc(1, 16, 32, 16, 8, act=a) for a in (wc.ACT_LEAKY, wc.ACT_TANH)] + [wc.wino_desc(1, 16, 32, 256, 8, act=wc.ACT_LEAKY)]
    return out


def test_restated_rules_match_the_library():
    from canonicalsg2im_amd._lib import lib
    descs = _sweep() + [c["d"] for c in CASES]
    seen = set()
    for d in descs:
        cd = to_ctypes(d)
        for fam, fn in (("f2", lib.csg_wino_conv_workspace), ("f4", lib.csg_wino4_conv_workspace)):
            want = wc.conv_workspace_bytes(fam, d)
            assert fn(cd) == want, (fam, d, want)
            seen.add((fam, (want > 0) - (want < 0)))
        for pad in (1, 2, 0, 3):
            want = wc.conv_workspace_bytes("f34", d, pad)
            assert lib.csg_wino34_conv_workspace(cd, pad) == want, ("f34", pad, d, want)
            seen.add(("f34", (want > 0) - (want < 0)))
            assert lib.csg_wino34_supported(cd, pad) == wc.wino34_supported(d, pad), (d, pad)
            if wc.wino_desc_check(d, 36, 0) == 0 and d["x_cs"] == d["Cin"] and lib.csg_wino34_supported(cd, pad):    # the planner's question is the narrower one:
                # maps from 15 pixels and 64 -> 32 channels up; what it says yes to, the plan serves
                assert want >= 0, (d, pad)
        for fam, fn in (("wg2", lib.csg_wino_bwd_weight_workspace), ("wg4", lib.csg_wino4_bwd_weight_workspace)):
            want = wc.wg_workspace_bytes(fam, d)
            assert fn(cd) == want, (fam, d, want)
            seen.add((fam, (want > 0) - (want < 0)))
        assert lib.csg_wino4_supported(cd) == wc.wino4_supported(d), d
        # "supported" asks about the shape only: where x is dense and y's stride is what the descriptor check admits, it is "workspace >= 0"
        if d["x_cs"] == d["Cin"] and d["y_cs"] % 4 == 0 and d["y_cs"] >= d["Cout"]:
            assert bool(lib.csg_wino4_supported(cd)) == (wc.conv_workspace_bytes("f4", d) >= 0), d
    assert seen == {(f, s) for f in ("f2", "f4", "f34") for s in (-1, 0, 1)} | {(f, s) for f in ("wg2", "wg4") for s in (-1, 1)}
    for (N, K) in ((4, 16), (32, 8), (33, 9), (100, 1296), (512, 32), (20, 12), (0, 8), (8, -1)):
        assert lib.csg_wino_pack_bytes(N, K) == wc.wino_pack_bytes(16, N, K)
        assert lib.csg_wino4_pack_bytes(N, K) == wc.wino_pack_bytes(36, N, K)


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_row_queries_match_the_library(c):
    """Per row: the workspace bytes and the pack bytes its launch is given, strided descriptors and the 0 of y_cs != Cout
    included."""
    from canonicalsg2im_amd._lib import lib
    d, cd, fam = c["d"], to_ctypes(c["d"]), c["fam"]
    if c["entry"] == "wgrad":
        fn = lib.csg_wino_bwd_weight_workspace if fam == "wg2" else lib.csg_wino4_bwd_weight_workspace
        p = wc.wg_plan(fam, d)
        assert fn(cd) == wc.wino_wg_workspace(d, p["nslab"]) > 0
        return
    got = {"f2": lambda: lib.csg_wino_conv_workspace(cd), "f4": lambda: lib.csg_wino4_conv_workspace(cd),
           "f34": lambda: lib.csg_wino34_conv_workspace(cd, c["pad"])}[fam]()
    assert got == wc.conv_workspace_bytes(fam, d, c["pad"])
    p, kind = wc.run_plan(c)
    if kind in ("split", "unsplit-short-workspace"):
        assert got == wc.conv_plan(fam, d, c["pad"], True)["ksplit"] * p["slab"] * 4 > 0
    if kind == "unsplit-strided-y":
        assert got == 0
    O, I, k, N, K = wc.pack_geometry(c)
    fn = lib.csg_wino_pack_bytes if fam == "f2" else lib.csg_wino4_pack_bytes
    assert fn(N, K) == wc.wino_pack_bytes(wc.POSITIONS[fam], N, K) > 0
    if fam == "f4":
        assert lib.csg_wino4_supported(cd) == 1


# ------------------------------------------------------------------------------------------------ the references
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _dense_conv_rows():
    return [c for c in SMALL if c["entry"] == "conv" and c["d"]["x_cs"] == c["d"]["Cin"] and c["d"]["y_cs"] == c["d"]["Cout"]]


@pytest.mark.parametrize("c", _dense_conv_rows(), ids=case_ids(_dense_conv_rows()))
def test_wino_ref64_is_torchs_float64_convolution(c):
    d, data = c["d"], wc.buffers(c)
    ref = wc.wino_ref64(c, data)
    assert bool(ref["own"].all())
    x, w = _nchw(data["x"].double()), data["w"].double()
    if c["sigma"]:
        w = w / data["sigma"].double()
    if c["bwd"]:
        # dX of y = conv(X, w, padding k - 1 - pad) for dY = x: autograd, not the flipped-weight formula
        k = w.shape[2]
        X = torch.zeros(d["B"], d["Cout"], *wc.out_size(c), dtype=torch.float64, requires_grad=True)
        F.conv2d(X, w, padding=k - 1 - c["pad"]).backward(x)
        v = X.grad
    else:
        v = F.conv2d(x, w, None if data["bias"] is None else data["bias"].double(), padding=c["pad"])
    slope = float(torch.tensor(d["slope"], dtype=torch.float32))
    v = F.leaky_relu(v, slope) if d["act"] == wc.ACT_LEAKY else (torch.tanh(v) if d["act"] == wc.ACT_TANH else v)
    if c["res"]:
        v = v + _nchw(data["res"].double())
    if c["gate"]:
        gs = float(torch.tensor(c["gate_slope"], dtype=torch.float32))
        v = v * torch.where(_nchw(data["gate"]) > 0, 1.0, gs).double()
        assert bool((data["gate"] == 0).any()) and bool((data["gate"] < 0).any())
    torch.testing.assert_close(_nchw(ref["y"]), v, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["f4_part_plain", "f4_part_mod"])
def test_part_reference_is_a_slice_of_the_whole_convolution(name):
    c = _one(name)
    d, data = c["d"], wc.buffers(c)
    xo, yo, t0 = c["x_off"], c["y_off"], 32 * c["part"]["tile_off"]
    whole = F.conv2d(_nchw(data["x"].double()[..., xo:xo + d["Cin"]]), data["w"].double(), data["bias"].double(), padding=1)
    v = whole[:, t0:t0 + d["Cout"]]
    if c["part"]["mod"]:
        go = c["part"]["g_off"]
        xh = (_nchw(data["mod_x"].double()[..., yo:yo + d["Cout"]]) - data["mean"].double()[None, :, None, None]) * data["invstd"].double()[None, :, None, None]
        v = F.leaky_relu(xh * (1 + _nchw(data["mod_gamma"].double()[..., go:go + d["Cout"]])) + v, float(torch.tensor(0.2, dtype=torch.float32)))
    ref = wc.wino_ref64(c, data)
    torch.testing.assert_close(_nchw(ref["y"][..., yo:yo + d["Cout"]]), v, rtol=1e-12, atol=1e-12)
    assert bool((ref["y"][~ref["own"]] == wc.SENTINEL).all())


def test_spade_reference_is_the_part_pair():
    """The joint launch's contract is the conv_part pair's: gamma = the first C outputs, then the modulated beta half.  At a
    small shape (the formula does not depend on whether the launch qualifies)."""
    sp = dict(gamma_out=True, gamma_cs=72, g_off=wc.OFF, mod_slope=0.2)
    c = dict(_one("f4_spade_gamma_out"), name="spade_small", d=wc.wino_desc(1, 16, 32, 16, 64, 16, 76), spade=sp)
    data = wc.buffers(c)
    ref = wc.wino_ref64(c, data)
    C, yo = 64, c["y_off"]
    gam = dict(c, entry="part", part=dict(tile_off=0, tiles_total=4, mod=False), d=dict(c["d"], y_cs=72))
    gdata = dict(data, y0=data["gamma0"], bias=data["bias"])
    g = wc.wino_ref64(gam, gdata)["y"]
    torch.testing.assert_close(g, ref["gamma_out"], rtol=0, atol=0)
    bet = dict(c, entry="part", part=dict(tile_off=2, tiles_total=4, mod=True, gamma_cs=72, g_off=wc.OFF, mod_slope=0.2))
    bdata = dict(data, mod_gamma=g)
    torch.testing.assert_close(wc.wino_ref64(bet, bdata)["y"], ref["y"], rtol=1e-13, atol=1e-13)
    assert bool((ref["y"][..., :yo] == wc.SENTINEL).all()) and bool((ref["gamma_out"][..., :wc.OFF] == wc.SENTINEL).all())


def _dense_wgrad_rows():
    return [c for c in WGRAD if c["d"]["x_cs"] == c["d"]["Cin"] and c["d"]["y_cs"] == c["d"]["Cout"]]


@pytest.mark.parametrize("c", _dense_wgrad_rows(), ids=case_ids(_dense_wgrad_rows()))
def test_wino_wgrad_ref64_is_torch_autograd(c):
    d, data = c["d"], wc.buffers(c)
    ref = wc.wino_wgrad_ref64(c, data)
    w = torch.zeros(d["Cout"], d["Cin"], 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(d["Cout"], dtype=torch.float64, requires_grad=True)
    F.conv2d(_nchw(data["x"].double()), w, b, padding=1).backward(_nchw(data["dy"].double()))
    torch.testing.assert_close(ref["dw"], w.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    if c["db"]:
        torch.testing.assert_close(ref["db"], b.grad, rtol=1e-12, atol=1e-12)
    else:
        assert ref["db"] is None


def _strided_rows():
    return [c for c in SMALL if c["d"]["x_cs"] != c["d"]["Cin"] or c["d"]["y_cs"] != c["d"]["Cout"]]


@pytest.mark.parametrize("c", _strided_rows(), ids=case_ids(_strided_rows()))
def test_strided_row_is_its_dense_twin(c):
    """The reference of a strided row equals the reference of the dense row on the same owned data, bit for bit; what the
    row does not own keeps the sentinel; what it may not read is NaN."""
    d, data = c["d"], wc.buffers(c)
    xo, yo = c["x_off"], c["y_off"]
    xs, ys = slice(xo, xo + d["Cin"]), slice(yo, yo + d["Cout"])
    dense = dict(c, d=dict(d, x_cs=d["Cin"], y_cs=d["Cout"]), x_off=0, y_off=0)
    dd = dict(data, x=data["x"][..., xs].contiguous())
    if xo:
        assert bool(torch.isnan(data["x"][..., :xo]).all()) and bool(torch.isnan(data["x"][..., xo + d["Cin"]:]).all())
    if c["entry"] == "wgrad":
        dd["dy"] = data["dy"][..., ys].contiguous()
        a, b = wc.reference(c, data), wc.reference(dense, dd)
        assert torch.equal(a["dw"], b["dw"]) and (a["db"] is None) == (b["db"] is None) and (a["db"] is None or torch.equal(a["db"], b["db"]))
        return
    for k in ("res", "gate", "mod_x", "y0"):
        if data.get(k) is not None:
            dd[k] = data[k][..., ys].contiguous()
            if yo and k != "y0":
                assert bool(torch.isnan(data[k][..., :yo]).all()) and bool(torch.isnan(data[k][..., yo + d["Cout"]:]).all())
    a, b = wc.reference(c, data), wc.reference(dense, dd)
    assert torch.equal(a["y"][..., ys], b["y"]) and bool(b["own"].all())
    assert bool((a["y"][~a["own"]] == wc.SENTINEL).all()) and int((~a["own"]).sum()) == a["y"].numel() - b["y"].numel()


# ------------------------------------------------------------------------------------------------ refusals before any device
FAKE = 0x10000000          # a 16-byte aligned address nothing dereferences: every refusal below returns before a launch


def _refused_call(lib, c):
    """The row's entry point with made-up addresses (the wrong one 4 bytes off): the return code."""
    d, fam, how = c["d"], c["fam"], c["how"]
    cd, P = to_ctypes(d), ctypes.c_void_p
    x, packed, y = (P(FAKE + 4 * (how == k)) for k in ("x", "packed", "y"))
    if how == "pack":
        fn = lib.csg_wino_pack_weights if fam == "f2" else lib.csg_wino4_pack_weights
        return fn(P(FAKE), 9 * d["Cin"], 9, 3, 1, d["Cout"], d["Cin"], 0, None, P(FAKE + 4), None)
    if c["entry"] == "wgrad":
        fn, q = ((lib.csg_wino_bwd_weight, lib.csg_wino_bwd_weight_workspace) if fam == "wg2" else
                 (lib.csg_wino4_bwd_weight, lib.csg_wino4_bwd_weight_workspace))
        return fn(cd, x, y, P(FAKE), P(FAKE), P(FAKE), q(cd) - 4, None)
    if c["entry"] == "part":
        pt = c["part"]
        return lib.csg_wino4_conv_part(cd, x, packed, pt["tile_off"], pt["tiles_total"], P(FAKE), None, None, 0, None, None, 1.0, y, None)
    if c["entry"] == "spade":
        return lib.csg_wino4_conv_spade(cd, x, packed, P(FAKE), P(FAKE), None, 0, P(FAKE), P(FAKE), 0.2, y, None)
    if fam == "f34":
        return lib.csg_wino34_conv(cd, c["pad"], x, packed, None, None, None, 0.0, y, None, 0, None)
    fn = lib.csg_wino_conv if fam == "f2" else lib.csg_wino4_conv
    return fn(cd, x, packed, None, None, None, 0.0, y, None, 0, None)


HOST_REFUSALS = [c for c in REFUSE if c["name"] != "refuse_f4_spade_unqualified"]     # that row's reason needs a device's CU count


@pytest.mark.parametrize("c", HOST_REFUSALS, ids=case_ids(HOST_REFUSALS))
def test_refusals_return_before_a_device_is_touched(c):
    """Every refusal row is decided on the host, ahead of the launch.  The addresses are made up, so this runs only where no
    launch can happen: with a device present the same rows run in tests/test_gpu_wino_paths.py on real buffers."""
    if torch.cuda.is_available():
        pytest.skip("a device is present: tests/test_gpu_wino_paths.py runs these rows on real buffers")
    from canonicalsg2im_amd._lib import last_error, lib
    code, text = c["refuse"]
    assert _refused_call(lib, c) == code, (c["name"], last_error())
    assert re.search(text, last_error()), (c["name"], last_error())
    if c["how"] is None and c["entry"] == "conv":                      # the descriptor itself: the query refuses too
        assert wc.conv_workspace_bytes(c["fam"], c["d"], c["pad"]) == -1
