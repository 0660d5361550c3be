"""The GEMM and few-output matrix on the CPU (tests/gemm_few_cases.py): the restated launch rules against the library's own
workspace and support queries (the library loads without a device; nothing is launched); the table's coverage of every launch
class, with each rule's boundary present on both sides; the references against torch's own float64 `linear` / `conv2d` and
their autograd; that the buffers the device test allocates contain every address a row can produce; and the conditions the
data must meet (the exact pass's bound, zeros among the gates, NaN where nothing may read, the entry row's kink clearance)."""
import inspect
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import gemm_few_cases as gc
from gemm_few_cases import CASES, ENTRY_CASES, REFUSALS, by_name, case_ids

NT = [c for c in CASES if c["kind"] == "nt"]
TN = [c for c in CASES if c["kind"] == "tn"]
FEW = [c for c in CASES if c["kind"] == "few"]
CINS = (32, 64, 128, 256, 512, 1024)


# ------------------------------------------------------------------------------------------------ the rules against the library
def _few_sweep():
    """Few-output descriptors across every rule's boundary: tiles around 1024 and 1536 / k, every Cin, OW 48 | 49, both
    kernel sizes, pixel counts around a block of the backward kernels."""
    out = []
    for B, cin, k in itertools.product((1, 2, 3, 300, 384, 400, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1535, 1536, 1537), CINS, (3, 4)):
        out.append(gc.few_desc(B, 4, 4, cin, k, k // 2, 1))
    out += [gc.few_desc(B, 1, 49, 64, 3, 1, 3) for B in (511, 512, 1023, 1024)]          # the wide tile on both sides of 1024 tiles
    for (ih, iw), cin, k in itertools.product(((8, 48), (9, 49), (17, 47), (18, 18), (7, 7), (33, 33), (40, 600), (32, 32), (32, 33), (1, 1024), (1, 1025)),
                                              CINS, (3, 4)):
        for pad in (0, 1, 2, 3):
            d = gc.few_desc(2, ih, iw, cin, k, pad, 2 if k == 4 else 3)
            if gc.few_supported(d) is None:
                out.append(d)
    return out


def test_restated_rules_match_the_library():
    from canonicalsg2im_amd._lib import lib
    shapes = {(r["M"], r["N"], r["K"]) for r in TN}
    for k in range(1, 41):
        for m in (256 * k - 1, 256 * k, 256 * k + 1):
            for n, kk in ((4, 4), (8, 8), (132, 4), (256, 128), (132, 260), (1152, 512), (4, 1156)):
                shapes.add((m, n, kk))
    shapes |= {(m, 4, 4) for m in (1, 16, 17, 31, 32, 33, 255)}
    forms = set()
    for M, N, K in sorted(shapes):
        p = gc.tn_plan(M, N, K)
        assert lib.csg_gemm_tn_workspace(M, N, K) == p["ws_bytes"], (M, N, K, p)
        assert p["rows_per"] % 32 == 0 and (p["nsplit"] - 1) * p["rows_per"] < M <= p["nsplit"] * p["rows_per"]
        forms.add("direct" if p["direct"] else gc.slab_sum_form(p["nsplit"]))
    assert forms == {"direct", "narrow", "wide"}
    assert lib.csg_gemm_tn_workspace(8, 6, 8) == -1 and lib.csg_gemm_tn_workspace(0, 4, 4) == -1
    seen = set()
    for d in _few_sweep() + [r["desc"] for r in FEW]:
        f, b = gc.few_fwd_plan(d), gc.few_bwd_plan(d)
        cd = gc.few_to_ctypes(d)
        assert lib.csg_conv_few_fwd_workspace(cd) == f["ws_bytes"], (d, f)
        assert lib.csg_conv_few_bwd_weight_workspace(cd) == b["ws_bytes"], (d, b)
        assert (f["ksplit"] - 1) * f["cps"] < f["nchunk"] <= f["ksplit"] * f["cps"] and 1 <= f["last_chunks"] <= f["cps"]
        assert (b["blocks"] - 1) * b["ppb"] < b["npix"] <= b["blocks"] * b["ppb"] and b["ppb"] % b["PL"] == 0
        assert b["opb"] * b["blocks"] >= b["nout"]                         # the db partition covers every output pixel
        seen.add((f["TX"], "split" if f["ksplit"] > 1 else "unsplit", gc.slab_sum_form(b["blocks"])))
    # (an unsplit forward has >= 1024 tiles, so its weight gradient has more than 16 blocks)
    assert seen == {(tx, "split", w) for tx in (16, 32) for w in ("narrow", "wide")} | {(16, "unsplit", "wide"), (32, "unsplit", "wide")}


def test_support_queries_agree_with_the_restated_conditions():
    from canonicalsg2im_amd._lib import last_error, lib
    rows = [dict(M=m, N=n, K=k, lda=k + pa, ldb=k + pb, ldy=n + py, ldg=n)
            for m, n, k in ((1, 4, 4), (8, 8, 6), (8, 6, 8), (8, 8, 8), (0, 4, 4), (129, 60, 36))
            for pa, pb, py in ((0, 0, 0), (4, 8, 12), (-4, 0, 0), (0, -4, 0), (0, 0, -4), (2, 0, 0), (0, 0, 2))]
    rows += NT + [r for r in REFUSALS if r["entry"] == "nt"]
    answers = set()
    for r in rows:
        want = gc.nt_supported(r["M"], r["N"], r["K"], r["lda"], r["ldb"], r["ldy"])
        assert lib.csg_gemm_supported(gc.nt_to_ctypes(r)) == int(want), r
        answers.add(want)
    assert answers == {True, False}
    assert not gc.nt_supported(**{k: by_name("refuse_nt_k6")[k] for k in ("M", "N", "K", "lda", "ldb", "ldy")})
    assert not gc.nt_supported(**{k: by_name("refuse_nt_lda")[k] for k in ("M", "N", "K", "lda", "ldb", "ldy")})
    g = by_name("refuse_nt_ldg")                                       # decided by the launch alone: the gate is no part of the query
    assert gc.nt_supported(g["M"], g["N"], g["K"], g["lda"], g["ldb"], g["ldy"]) and g["ldg"] < g["N"] and g["gated"]
    descs = [gc.few_desc(2, 8, 8, cin, k, 1, n, x_cs=cin + xp, KW=kw) for cin in (16, 32, 96, 128, 384, 1024, 2048) for k, kw in ((3, 3), (4, 4), (5, 5), (3, 4))
             for n in (0, 1, 2, 3, 4, 5) for xp in (0, 8, 2, -4)]
    descs += [gc.few_desc(1, 1, 1, 32, 3, 0, 1)] + [r["desc"] for r in FEW] + [r["desc"] for r in REFUSALS if "desc" in r]
    answers = set()
    for d in descs:
        why = gc.few_supported(d)
        assert lib.csg_conv_few_supported(gc.few_to_ctypes(d)) == int(why is None), d
        if why is not None:
            assert re.search(why, last_error()), (d, why, last_error())
        answers.add(why)
    assert len(answers) == 6                                            # served, and each of the five refusals
    for r in REFUSALS:
        if r["entry"] == "few_fwd":
            assert gc.few_supported(r["desc"]) == r["text"], r["name"]
        elif "desc" in r:
            assert gc.few_supported(r["desc"]) is None, r["name"]


def test_grid_remap_is_a_bijection_for_every_grid_size():
    for n in list(range(1, 700)) + [1023, 1024, 1025, 4097]:
        assert sorted(gc.xcd_remap(b, n) for b in range(n)) == list(range(n)), n


# ------------------------------------------------------------------------------------------------ coverage
NT_CLASSES = {(64, "plain", "1 partial"), (64, "plain", "1 full"), (64, "gated", "2 with tail"), (64, "gated", "odd"), (64, "plain", "even"),
              (128, "plain", "1 full"), (128, "gated", "2 with tail"), (128, "gated", "odd"), (128, "gated", "even"),
              (128, "plain", "1 partial"), (128, "plain", "even")}
TN_CLASSES = {("direct", "nodb", "tails"), ("direct", "db", "tails"), ("narrow", "db", "tails"), ("narrow", "nodb", "whole"),
              ("wide", "db", "tails")}
FEW_FWD_CLASSES = {
    (16, "even", "remainder", (3, 4)), (16, "even", "remainder", (3, 1)), (16, "even", "remainder", (3, 2)), (16, "even", "remainder", (3, 3)),
    (16, "even", "fours + remainder", (3, 1)), (16, "even", "remainder", (4, 2)), (16, "even", "remainder", (4, 1)),
    (16, "even", "fours + remainder", (4, 1)), (32, "even", "remainder", (3, 3)), (16, "uneven", "fours + remainder", (3, 2)),
    (16, "unsplit", "none", (3, 3)), (16, "refused", "none", (4, 1)), (16, "even", "fours + remainder", (3, 3))}
FEW_BWD_CLASSES = {(32, "one", "image", "narrow"), (1, "many", "in row", "narrow"), (32, "many", "in row", "narrow"), (2, "many", "in row", "narrow"),
                   (16, "one", "in row", "narrow"), (8, "many", "in row", "narrow"), (1, "many", "in row", "wide"), (16, "many", "image", "wide"),
                   (8, "many", "row", "wide"), (4, "one", "in row", "narrow"), (32, "many", "in row", "wide")}


def test_table_names_every_launch_class():
    names = case_ids() + [r["name"] for r in REFUSALS] + [e["name"] for e in ENTRY_CASES]
    assert len(set(names)) == len(names)
    assert {gc.nt_class(r) for r in NT} == NT_CLASSES
    assert {gc.tn_class(r) for r in TN} == TN_CLASSES
    assert {gc.few_fwd_class(r) for r in FEW} == FEW_FWD_CLASSES
    assert {gc.few_bwd_class(r) for r in FEW if "wgrad" in r["dirs"]} == FEW_BWD_CLASSES
    # nt: both tiles x plain | gated x every stage count class; grids with the residues mod 8 the rows name
    for tile in (64, 128):
        assert {k for t, _, k in NT_CLASSES if t == tile} == {"1 partial", "1 full", "2 with tail", "odd", "even"}, tile
        assert {g for t, g, _ in NT_CLASSES if t == tile} == {"plain", "gated"}, tile
    grids = [gc.nt_plan(r["M"], r["N"], r["K"])["grid"] for r in NT]
    assert set(grids) == {1, 2, 3, 6, 9, 17} and {g % 8 for g in grids} == {1, 2, 3, 6}
    # few forward: every template instance of FEW_DISPATCH, every way of cutting the channels, both finish loops, both tiles
    assert {c[3] for c in FEW_FWD_CLASSES} == {(3, 1), (3, 2), (3, 3), (3, 4), (4, 1), (4, 2)}
    assert {c[1] for c in FEW_FWD_CLASSES} == {"unsplit", "even", "uneven", "refused"} and {c[0] for c in FEW_FWD_CLASSES} == {16, 32}
    assert {c[2] for c in FEW_FWD_CLASSES} == {"none", "remainder", "fours + remainder"}
    assert {gc.few_fwd_class(r)[3] for r in FEW if "wgrad" in r["dirs"]} == {(3, 1), (3, 2), (3, 3), (3, 4), (4, 1), (4, 2)}   # backward too
    # few backward: every PL, one | many blocks, a step longer than a row and than an image, both slab sums
    assert {c[0] for c in FEW_BWD_CLASSES} == {1, 2, 4, 8, 16, 32} and {c[1] for c in FEW_BWD_CLASSES} == {"one", "many"}
    assert {c[2] for c in FEW_BWD_CLASSES} == {"in row", "row", "image"} and {c[3] for c in FEW_BWD_CLASSES} == {"narrow", "wide"}
    assert {r["name"] for r in REFUSALS} == {"refuse_nt_k6", "refuse_nt_lda", "refuse_nt_ldg", "refuse_tn_short_ws", "refuse_few_5x5",
                                             "refuse_few_cin96", "refuse_few_4x4_n3", "refuse_few_wgrad_short_ws"}
    assert sum(not r["bias"] for r in FEW) == 1 and sum(r["desc"]["act"] == gc.ACT_LEAKY for r in FEW) == 1
    assert {r["name"] for r in FEW if r["desc"]["x_cs"] == r["desc"]["Cin"] + 8} == {"few_head_xcs", "few_ow49_xcs"}


def test_every_rule_boundary_is_present_on_both_sides():
    """Typed-in expectations: a changed constant in the restated rules, or a row whose shape drifted, fails here."""
    nt = {r["name"]: gc.nt_plan(r["M"], r["N"], r["K"]) for r in NT}
    want = {"nt_one": (64, 32, 1, 1, 1), "nt_narrow_exact": (64, 32, 1, 0, 1), "nt_narrow_tail": (64, 32, 2, 1, 2), "nt_narrow_odd": (64, 32, 3, 0, 3),
            "nt_narrow_long": (64, 32, 36, 0, 1), "nt_wide_first": (128, 16, 1, 0, 2), "nt_wide_tail": (128, 16, 2, 1, 6),
            "nt_wide_odd": (128, 16, 3, 0, 1), "nt_wide_grid9": (128, 16, 4, 0, 9), "nt_wide_grid17": (128, 16, 1, 1, 17),
            "nt_wide_long": (128, 16, 72, 0, 2)}
    assert {n: (p["tile"], p["bk"], p["nstage"], p["tail_slots"], p["grid"]) for n, p in nt.items()} == want
    assert {by_name(n)["N"] for n in ("nt_narrow_exact", "nt_narrow_odd")} == {64} and by_name("nt_wide_first")["N"] == 68      # N 64 | 68
    assert by_name("nt_one")["M"] == 1 and by_name("nt_wide_odd")["M"] == 127
    for n in ("nt_narrow_tail", "nt_wide_tail"):
        r = by_name(n)
        pads = (r["lda"] - r["K"], r["ldb"] - r["K"], r["ldy"] - r["N"], r["ldg"] - r["N"])
        assert len(set(pads)) == 4 and all(p > 0 and p % 4 == 0 for p in pads), n
    tn = {r["name"]: gc.tn_plan(r["M"], r["N"], r["K"]) for r in TN}
    want = {"tn_one_row": (1, 32, 1), "tn_17_rows": (1, 32, 17), "tn_k_tiles": (1, 512, 511), "tn_two": (2, 288, 232), "tn_two_ragged": (2, 352, 348),
            "tn_four": (4, 288, 166), "tn_15": (15, 288, 68), "tn_16": (16, 256, 256), "tn_17": (17, 256, 256), "tn_29": (29, 288, 136)}
    assert {n: (p["nsplit"], p["rows_per"], p["last_rows"]) for n, p in tn.items()} == want
    assert (tn["tn_17_rows"]["last_stages"], tn["tn_17_rows"]["last_stage_rows"]) == (2, 1) and tn["tn_two"]["last_stage_rows"] == 8
    assert [gc.slab_sum_form(tn[n]["nsplit"]) for n in ("tn_15", "tn_16", "tn_17")] == ["narrow", "wide", "wide"]
    per = (17 + 3) >> 2                                                # k_slab_reduce<1>: quarters of 5, 5, 5, 2 at 17 slabs
    assert [min(17, (w + 1) * per) - w * per for w in range(4)] == [5, 5, 5, 2]
    assert gc.cdiv(by_name("tn_k_tiles")["K"], 128) == 3 and by_name("tn_k_tiles")["K"] % 128 == 4
    ff = {r["name"]: gc.few_fwd_plan(r["desc"]) for r in FEW}
    want = {"few_tiny": (16, 3, 1, 2, 1), "few_1024": (16, 2, 1, 64, 1), "few_4x4_32": (16, 9, 1, 2, 1), "few_head": (16, 8, 1, 32, 1),
            "few_ow49": (32, 4, 1, 4, 1), "few_ow48": (16, 3, 1, 4, 1), "few_ow48_4x4": (16, 6, 1, 8, 1), "few_uneven": (16, 300, 11, 6, 9),
            "few_unsplit": (16, 1100, 4, 1, 4), "few_split4": (16, 400, 2, 4, 2), "few_bigpad": (16, 2, 1, 16, 1), "few_wide_map": (32, 95, 1, 2, 1)}
    assert {n: (ff[n]["TX"], ff[n]["tiles"], ff[n]["cps"], ff[n]["ksplit"], ff[n]["last_chunks"]) for n in want} == want
    assert (gc.few_out(by_name("few_ow49")["desc"])[1], gc.few_out(by_name("few_ow48")["desc"])[1], gc.few_out(by_name("few_ow48_4x4")["desc"])[1]) == (49, 48, 48)
    assert (ff["few_1024"]["fours"], ff["few_1024"]["rem"]) == (15, 3) and (ff["few_uneven"]["fours"], ff["few_uneven"]["rem"]) == (1, 1)
    assert (ff["few_split4"]["fours"], ff["few_split4"]["rem"]) == (0, 3) and ff["few_ow49"]["ragged"] and ff["few_wide_map"]["ragged"]
    d = by_name("few_bigpad")["desc"]
    assert d["pad"] > d["KH"] - 1 - d["pad"] + 1 and gc.few_out(d) == (10, 14)            # output rows that see only padding
    fb = {r["name"]: gc.few_bwd_plan(r["desc"]) for r in FEW}
    want = {"few_tiny": (32, 1, 75), "few_1024": (1, 4, 2), "few_4x4_32": (32, 2, 65), "few_head": (2, 11, 8), "few_ow49": (16, 1, 441),
            "few_ow48_4x4": (8, 4, 31), "few_uneven": (1, 150, 32), "few_unsplit": (16, 20, 172), "few_split4": (8, 40, 16),
            "few_wide_map": (32, 24, 448)}
    assert {n: (fb[n]["PL"], fb[n]["blocks"], fb[n]["last_pixels"]) for n in want} == want and fb["few_split4"]["ppb"] == 256
    for r in FEW:                                                       # db's partition is not the input pixels' partition
        assert fb[r["name"]]["opb"] * fb[r["name"]]["blocks"] >= fb[r["name"]]["nout"], r["name"]
    assert fb["few_head"]["opb"] != fb["few_head"]["ppb"]
    # the entry rows: wide tile, then narrow, a gated wide backward-data, a narrow one
    k0, k1, k2 = ENTRY_CASES[0]["dims"]
    assert [gc.nt_plan(257, n, k)["tile"] for n, k in ((k1, k0), (k2, k1), (k1, k2), (k0, k1))] == [128, 64, 128, 64]
    e = ENTRY_CASES[1]
    assert gc.nt_plan(e["B"] * e["H"] * e["W"], e["Cout"], e["Cin"])["tile"] == 128 and gc.nt_plan(234, e["Cin"], e["Cout"])["tile"] == 64


# ------------------------------------------------------------------------------------------------ the references against torch
def _close(name, got, ref):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert scale > 0 and err <= 1e-12 * scale, "%s: %.3e of scale %.3e" % (name, err, scale)


@pytest.mark.parametrize("c", NT, ids=case_ids(NT))
def test_nt_ref_is_torchs_linear(c):
    data = gc.make_data(c, "random")
    got = gc.nt_ref(c, data)["y"]
    M, N, K = c["M"], c["N"], c["K"]
    v = F.linear(data["a"][:, :K].double(), data["bw"][:, :K].double(), None if data["bias"] is None else data["bias"].double())
    if c["act"] == gc.ACT_LEAKY:
        v = F.leaky_relu(v, float(torch.tensor(c["slope"], dtype=torch.float32)))
    if c["gated"]:
        gate = data["gate"][:, :N]
        v = v * ((gate > 0).double() + (gate <= 0).double() * c["gate_slope"])
    assert tuple(got.shape) == (M, N)
    _close(c["name"], got, v)


@pytest.mark.parametrize("c", TN, ids=case_ids(TN))
def test_tn_ref_is_torchs_weight_gradient(c):
    data = gc.make_data(c, "random")
    got = gc.tn_ref(c, data)
    x = data["x"][:, :c["K"]].double()
    w = torch.zeros(c["N"], c["K"], dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c["N"], dtype=torch.float64, requires_grad=True)
    dw, db = torch.autograd.grad(F.linear(x, w, b), (w, b), data["dy"][:, :c["N"]].double())
    _close(c["name"] + " dw", got["dw"], dw)
    if c["db"]:
        _close(c["name"] + " db", got["db"], db)
    else:
        assert got["db"] is None


@pytest.mark.parametrize("c", FEW, ids=case_ids(FEW))
def test_few_ref_is_torchs_convolution(c):
    d, data, n = c["desc"], gc.make_data(c, "random"), c["desc"]["cout_real"]
    got = gc.few_ref(c, data)
    OH, OW = gc.few_out(d)
    x = data["x"][..., :d["Cin"]].double().permute(0, 3, 1, 2)
    if d["in_act"]:
        x = F.leaky_relu(x, float(torch.tensor(d["in_slope"], dtype=torch.float32)))
    w = data["w"][:n].double().permute(0, 3, 1, 2)
    y = F.conv2d(x, w, None, 1, d["pad"])
    if c["bias"]:
        y = y + data["bias"][:n].double().view(1, n, 1, 1)
    y = {gc.ACT_NONE: y, gc.ACT_LEAKY: F.leaky_relu(y, float(torch.tensor(d["slope"], dtype=torch.float32))), gc.ACT_TANH: torch.tanh(y)}[d["act"]]
    gy = data["dy"][..., :n].double().permute(0, 3, 1, 2)
    assert tuple(got["y"].shape) == (d["B"], OH, OW, 4) and tuple(got["dx"].shape) == (d["B"], d["IH"], d["IW"], d["Cin"])
    _close(c["name"] + " y", got["y"][..., :n].permute(0, 3, 1, 2), y)
    _close(c["name"] + " dx", got["dx"].permute(0, 3, 1, 2), torch.nn.grad.conv2d_input(x.shape, w, gy, 1, d["pad"]))
    _close(c["name"] + " dw", got["dw"][:n].permute(0, 3, 1, 2), torch.nn.grad.conv2d_weight(x, w.shape, gy, 1, d["pad"]))
    _close(c["name"] + " db", got["db"][:n], gy.sum((0, 2, 3)))
    for t in (got["y"][..., n:], got["dw"][n:], got["db"][n:]):
        assert bool((t == 0).all()), c["name"]


def test_entry_refs_are_torchs_autograd():
    for e in ENTRY_CASES:
        data = gc.entry_data(e, "random")
        ref = gc.entry_ref(e, data)
        if e["kind"] == "linear":
            h = torch.clamp(data["x"].double() @ data["w1"].double().t() + data["b1"].double(), min=0)
            _close(e["name"], ref["y"], h @ data["w2"].double().t() + data["b2"].double())
            _close(e["name"] + " db2", ref["db2"], data["gy"].double().sum(0))
            _close(e["name"] + " dw2", ref["dw2"], data["gy"].double().t() @ h)
        else:
            x2 = data["x"].double().permute(0, 2, 3, 1).reshape(-1, e["Cin"])
            y2 = ref["y"].permute(0, 2, 3, 1).reshape(-1, e["Cout"])
            _close(e["name"], y2, x2 @ data["w"].double().view(e["Cout"], e["Cin"]).t())


# ------------------------------------------------------------------------------------------------ addresses
@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_every_address_lies_inside_the_rows_buffers(c):
    numel = {k: int(torch.Size(s).numel()) for k, s in gc.buffers(c).items()}
    if c["kind"] == "nt":
        M, N, K = c["M"], c["N"], c["K"]
        assert gc.nt_supported(M, N, K, c["lda"], c["ldb"], c["ldy"]) and c["ldg"] % 4 == 0 and c["ldg"] >= N
        assert (M - 1) * c["lda"] + K <= numel["a"] and (N - 1) * c["ldb"] + K <= numel["bw"] and N <= numel["bias"]
        assert (M - 1) * c["ldg"] + N <= numel["gate"] and (M - 1) * c["ldy"] + N <= numel["y"]
        p = gc.nt_plan(M, N, K)
        assert p["grid"] == gc.cdiv(M, 128) * p["nnb"] and p["nnb"] * p["tile"] >= N and p["nstage"] * p["bk"] >= K
    elif c["kind"] == "tn":
        M, N, K = c["M"], c["N"], c["K"]
        assert N % 4 == 0 and K % 4 == 0 and c["ldy"] % 4 == 0 and c["ldx"] % 4 == 0 and c["ldy"] >= N and c["ldx"] >= K
        assert (M - 1) * c["ldy"] + N <= numel["dy"] and (M - 1) * c["ldx"] + K <= numel["x"] and N * K == numel["dw"] and N == numel["db"]
        p = gc.tn_plan(M, N, K)
        assert (0 if p["direct"] else p["nsplit"] * (N * K + N)) == numel["ws"]
        assert p["rows_per"] * max(c["ldy"], c["ldx"]) * 4 < 2 ** 31 - 4096
    else:
        d = c["desc"]
        assert gc.few_supported(d) is None, c["name"]
        OH, OW = gc.few_out(d)
        f, b = gc.few_fwd_plan(d), gc.few_bwd_plan(d)
        assert (b["npix"] - 1) * d["x_cs"] + d["Cin"] <= numel["x"] == numel["dx"] and f["nchunk"] * gc.FW_CK == d["Cin"]
        assert b["nout"] * 4 == numel["y"] == numel["dy"] and 4 * d["KH"] * d["KW"] * d["Cin"] == numel["w"] == numel["dw"]
        assert numel["ws_fwd"] == (f["ksplit"] * b["nout"] * 4 if f["ksplit"] > 1 else 0)
        assert numel["ws_wgrad"] == b["blocks"] * (numel["dw"] + 4)
        assert (f["TY"] + d["KH"] - 1) * (f["TX"] + d["KW"] - 1) * (gc.FW_CK // 4) <= 7 * 256        # the forward's staging registers
        assert (f["TY"] + d["KH"] - 1) * (f["TX"] + d["KW"] - 1) * 20 * 4 <= 96 * 1024                # and its LDS patch
    assert all(n * 4 < 2 ** 31 for n in numel.values())


# ------------------------------------------------------------------------------------------------ the data
@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_data_conditions(c):
    """The exact pass: integers in [-2, 2], power-of-two slopes, no tanh, and a bound on every partial sum that leaves two
    bits for the quarter units the slopes introduce.  Both passes: NaN exactly where no kernel may read; gated rows carry
    exact zeros of both signs in at least a quarter of the gate."""
    assert 4 * gc.exact_bound(c) < 2 ** 24, c["name"]
    ex = gc.row_for(c, "exact")
    if c["kind"] == "nt":
        assert ex["slope"] in (0.0, 0.25, 0.5) and ex["gate_slope"] == 0.5
    elif c["kind"] == "few":
        assert ex["desc"]["act"] != gc.ACT_TANH and ex["desc"]["slope"] in (0.0, 0.25, 0.5) and ex["desc"]["in_slope"] in (0.0, 0.25, 0.5)
        assert gc.row_for(c, "random") is c
    for kind in gc.KINDS:
        data = gc.make_data(c, kind)
        for name, t in data.items():
            if t is None:
                continue
            assert t.dtype == torch.float32 and tuple(t.shape) == tuple(gc.buffers(c)[name]), (c["name"], name)
            live = torch.isfinite(t)
            if kind == "exact":
                v = t[live]
                ok = (v == v.round()) & (v.abs() <= 2)
                if name == "gate":
                    ok = torch.ones_like(ok)
                if name == "dy" and c["kind"] == "few":
                    ok = ok | (v == gc.DY_PAD)
                assert bool(ok.all()), (c["name"], name)
        if c["kind"] == "nt":
            K, N = c["K"], c["N"]
            assert bool(torch.isfinite(data["a"][:, :K]).all()) and bool(torch.isnan(data["a"][:, K:]).all())
            assert bool(torch.isfinite(data["bw"][:, :K]).all()) and bool(torch.isnan(data["bw"][:, K:]).all())
            assert (data["gate"] is not None) == c["gated"] and (data["bias"] is not None) == c["bias"]
            if c["gated"]:
                gate = data["gate"][:, :N]
                assert bool(torch.isnan(data["gate"][:, N:]).all()) and bool(torch.isfinite(gate).all())
                zero, neg = gate == 0, torch.signbit(gate)
                assert float(zero.float().mean()) >= 0.25 and bool((zero & neg).any()) and bool((zero & ~neg).any())
                assert bool((gate > 0).any()) and bool((gate < 0).any())
        elif c["kind"] == "tn":
            assert bool(torch.isnan(data["dy"][:, c["N"]:]).all()) and bool(torch.isnan(data["x"][:, c["K"]:]).all())
            assert bool(torch.isfinite(data["dy"][:, :c["N"]]).all()) and bool(torch.isfinite(data["x"][:, :c["K"]]).all())
        else:
            d = c["desc"]
            assert bool(torch.isnan(data["x"][..., d["Cin"]:]).all()) and bool(torch.isfinite(data["x"][..., :d["Cin"]]).all())
            assert bool(torch.isnan(data["w"][d["cout_real"]:]).all()) and bool(torch.isfinite(data["w"][:d["cout_real"]]).all())
            assert bool((data["dy"][..., d["cout_real"]:] == gc.DY_PAD).all())
            assert (data["bias"] is not None) == c["bias"]
            if c["bias"]:
                assert bool(torch.isnan(data["bias"][d["cout_real"]:]).all()) and bool(torch.isfinite(data["bias"][:d["cout_real"]]).all())
    if c["name"] in gc.SPLIT_TWIN:
        twin = gc.make_data(by_name(gc.SPLIT_TWIN[c["name"]]), "random")
        assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(twin[k])) for k, a in gc.make_data(c, "random").items())


def test_entry_rows_keep_clear_of_the_kink():
    e = ENTRY_CASES[0]
    data = gc.entry_data(e, "random")
    for t in (torch.float32, torch.float64):
        pre = F.linear(data["x"].to(t), data["w1"].to(t), data["b1"].to(t))
        assert float(pre.abs().min()) >= gc.KINK_CLEARANCE, t
        assert bool((pre > 0).any()) and bool((pre < 0).any())
    assert gc.entry_clearance(data) >= gc.KINK_CLEARANCE
    assert torch.equal(data["x"], gc.entry_data(e, "random")["x"])     # the same seed every time
    ex = gc.entry_data(e, "exact")
    assert all(bool((v == v.round()).all()) and float(v.abs().max()) <= 2 for v in ex.values())
    k0, k1, k2 = e["dims"]
    hidden, dpre = 4 * k0 + 2, 4 * k2                                  # the largest partial sums of the exact pass, layer by layer
    assert 4 * max(2 * hidden * k1 + 2, 2 * hidden * e["M"], 2 * dpre * k1, 2 * dpre * e["M"]) < 2 ** 24
    c = ENTRY_CASES[1]
    assert 4 * max(4 * c["Cin"], 4 * c["Cout"], 4 * c["B"] * c["H"] * c["W"]) < 2 ** 24


def test_no_reads_from_outside_the_repository():
    for mod in (gc, __import__("test_gpu_gemm_few_paths")):
        src = inspect.getsource(mod)
        assert not re.search(r"""["'](/|~|\.\./)[A-Za-z_.]""", src), mod.__name__
        assert set(re.findall(r"environ[^\n]*?[\"']([A-Z_]+)[\"']", src)) <= {"GEMM_FEW_PATHS_REPORT"}, mod.__name__
    assert os.path.dirname(os.path.abspath(gc.__file__)) == os.path.dirname(os.path.abspath(__file__))
