"""The scene-graph encoder matrix on the CPU (tests/graph_cases.py): the table's coverage of every value the restated
dispatch rules can return, with each boundary present on both sides; `graph_ref64` against the golden file the reference's
own GraphTripleConv wrote; the host CSR loop against a second construction; the rows' own conditions; the restated rules
against the library's workspace queries (the library loads without a device)."""
import inspect
import os
import re

import pytest
import torch

import graph_cases as gc
from conftest import load_golden
from graph_cases import CASES, case_ids

RUN = [c for c in CASES if not c["refuse"]]
CSR = [c for c in RUN if c["family"] == "csr"]
SEG = [c for c in RUN if c["family"] == "seg"]
EMB = [c for c in RUN if c["family"] == "embed"]
LAYER = [c for c in RUN if c["family"] == "layer"]


def _one(name):
    (c,) = [c for c in CASES if c["name"] == name]
    return c


def _field(c, key):
    """`key=value` of a row's computed kernels string."""
    m = re.search(r"(?:^| )%s=(\S+)" % re.escape(key), c["kernels"])
    return m.group(1) if m else None


def _parts(c):
    """{"pooled" | "dobj": (LPE, passes, finish)} of a seg row's kernels string."""
    return {m.group(1): (int(m.group(2)), int(m.group(3)), m.group(4))
            for m in re.finditer(r"(pooled|dobj):LPE=(\d+)x(\d+) finish=(\w+)", c["kernels"])}


def test_dispatch_boundaries_are_present_on_both_sides():
    """Typed-in expectations: a changed constant in the restated rules (or a deleted row) fails here."""
    names = case_ids()
    assert len(set(names)) == len(names)
    # ---- the CSR builder: O <= 254 && 512 <= T <= 65535 && lds <= 150 KB, O <= 1024
    want = {"csr_o5_t511": "plain", "csr_o5_t512": "sorted", "csr_o3_t65535": "sorted", "csr_o3_t65536": "plain",
            "csr_o254_t600": "sorted", "csr_o255_t600": "plain", "csr_o254_t45000": "plain", "csr_o300_t2048": "plain",
            "csr_o300_t2049": "plain", "csr_o1024_t300": "plain", "csr_o1_t513": "sorted", "csr_o4_t0": "plain",
            "csr_bad_o40_t700": "sorted", "csr_bad_o300_t700": "plain", "refuse_csr_o1025": "refuse"}
    for name, b in want.items():
        c = _one(name)
        assert _field(c, "csr") == b == gc.csr_builder(c["O"], c["T"]), name
    assert {(c["O"], c["T"]) for c in CASES if c["family"] == "csr"} >= {
        (5, 511), (5, 512), (3, 65535), (3, 65536), (254, 600), (255, 600), (254, 45000), (300, 2048), (300, 2049), (1024, 300),
        (1, 513), (4, 0), (40, 700), (300, 700), (1025, 300)}
    lds = _one("csr_o254_t45000")
    assert 512 <= lds["T"] <= 65535 and lds["O"] <= 254 and gc.csr_sorted_lds(lds["T"], lds["O"]) > 150 * 1024   # the LDS limit alone
    assert gc.csr_sorted_lds(65535, 3) <= 150 * 1024 and gc.csr_sorted_lds(600, 254) <= 150 * 1024
    assert (_field(_one("csr_o300_t2048"), "stage"), _field(_one("csr_o300_t2049"), "stage")) == ("1", "2")
    assert _field(_one("csr_o1024_t300"), "slots") == "4" and _field(_one("csr_o4_t0"), "stage") == "0"
    assert _one("refuse_csr_o1025")["refuse"] and _one("refuse_csr_o1025")["O"] == 1025
    assert [c for c in CSR if c["bad"] and _field(c, "csr") == "sorted"] and [c for c in CSR if c["bad"] and _field(c, "csr") == "plain"]
    # ---- sparse | edge-balanced: deg = ceil(2T / O) <= 48
    for relu in ("relu", "plain"):
        assert _field(_one("seg_o8_t192_" + relu), "rowsum") == "sparse" and _field(_one("seg_o8_t193_" + relu), "rowsum") == "dense"
    assert gc.rowsum_nseg(8, 192) == 0 and gc.rowsum_nseg(8, 193) == gc.cdiv(386, 128) + 8
    assert gc.rowsum_nseg(1025, 10 ** 6) == 0
    # ---- segments of a row: 128 | 129 edges, an empty row keeps one
    assert (gc.row_segments(0), gc.row_segments(128), gc.row_segments(129)) == (1, 1, 2)
    for relu in ("relu", "plain"):
        c = _one("seg_deg_128_129_0_" + relu)
        assert _field(c, "rowsum") == "dense" and c["degrees"][:3] == (128, 129, 0) and _field(c, "maxS") == "2"
        assert bool((gc.row_lengths(gc.make_data(c)["tr"], c["O"])[:, :3] == torch.tensor([128, 129, 0])).all())
    # ---- lanes per edge, d0 passes, finish groups
    assert [gc.rowsum_lpe(D) for D in (4, 8, 12, 16, 128, 512, 516, 1024, 1028, 2048)] == [1, 2, 4, 4, 32, 128, 256, 256, 256, 256]
    assert [gc.rowsum_passes(D) for D in (4, 12, 1024, 1028, 2048)] == [1, 1, 1, 2, 2]
    assert (gc.finish_groups(256), gc.finish_groups(32), gc.finish_groups(1)) == (4, 32, 1024)
    for relu in ("relu", "plain"):
        assert _parts(_one("seg_star_o6_t4200_h128_" + relu))["pooled"] == (32, 1, "pairs")          # 66 segments, 32 groups
        assert _parts(_one("seg_star_o6_t600_h516_" + relu))["pooled"] == (256, 1, "pairs")          # 10 segments, 4 groups
    # ---- embedding chunks: clamp(8192 / dim, 32, 1024) rows
    assert [gc.emb_chunk_rows(d) for d in (4, 8, 9, 32, 128, 256, 300)] == [1024, 1024, 910, 256, 64, 32, 32]
    want = {"emb_8x8_r1024": (1024, 1, 1), "emb_8x8_r1025": (1024, 2, 1), "emb_179x128_r300": (64, 5, 90),
            "emb_4x256_r70": (32, 3, 4), "emb_8x32_r27000": (256, 106, 1)}
    for name, (chunk, chunks, gy) in want.items():
        assert _one(name)["kernels"] == "chunk=%d chunks=%d gridy=%d" % (chunk, chunks, gy), name
    assert _one("refuse_emb_dim300")["kernels"] == "refuse" and _one("emb_dim300_fwd")["kernels"] == "fwd"
    assert gc.emb_rule(10, 6, 256)["refuse"] is False and gc.emb_rule(10, 6, 257)["refuse"] is True


def test_table_covers_every_value_the_rules_return():
    for c in CASES:                                                   # `kernels` is what the rules give, not what was typed
        d = dict(tr=gc.make_data(c)["tr"]) if c["family"] in ("seg", "layer") else None
        assert c["kernels"] == gc._kernels(c, d), c["name"]
    assert {c["family"] for c in RUN} == {"csr", "seg", "embed", "mask", "layer"}
    assert {_field(c, "csr") for c in CASES if c["family"] == "csr"} == {"sorted", "plain", "refuse"}
    assert {_field(c, "csr") for c in SEG} == {"sorted", "plain"}
    assert {_field(c, "rowsum") for c in SEG} == {"sparse", "dense"}
    for part in ("pooled", "dobj"):
        assert {_parts(c)[part][2] for c in SEG if part in _parts(c)} == {"none", "idle", "single", "pairs"} - (
            {"pairs"} if part == "dobj" else set()), part
    # every LPE and two d0 passes, in both launch modes (the weighted kernel: pooled)
    for mode in ("sparse", "dense"):
        got = {_parts(c)["pooled"][:2] for c in SEG if _field(c, "rowsum") == mode}
        assert got >= {(1, 1), (4, 1), (8, 1), (256, 2)}, (mode, got)
    assert {_parts(c)["pooled"][0] for c in SEG} >= {1, 4, 32, 256}
    assert {_parts(c)["dobj"][0] for c in SEG if "dobj" in _parts(c)} >= {1, 2, 4}
    assert [c for c in SEG if c["H"] == 12 and c["Din"] == 12] and [c for c in SEG if c["H"] == 2048 and c["Din"] == 12]
    assert [c for c in SEG if c["H"] > 256 and c["H"] % 256 == 4] and [c for c in SEG if c["Dp"] > 256]   # k_segment_avg_bwd: 2nd pass
    # h_is_relu both ways on the launch-rule rows; every builder; the corner rows
    for stem in ("seg_o8_t192", "seg_o8_t193", "seg_deg_128_129_0", "seg_star_o6_t4200_h128", "seg_star_o6_t600_h516"):
        a, b = _one(stem + "_relu"), _one(stem + "_plain")
        assert a["relu"] and not b["relu"] and {k: v for k, v in a.items() if k not in ("name", "relu", "kernels")} == {
            k: v for k, v in b.items() if k not in ("name", "relu", "kernels")}
    assert {c["graph"] for c in SEG} == set(gc.GRAPHS)
    for mode in ("sparse", "dense"):
        assert [c for c in SEG if c["graph"] == "padded" and c["B"] == 3 and _field(c, "rowsum") == mode], mode
        assert [c for c in SEG if c["zero_conf"] is not None and _field(c, "rowsum") == mode], mode
        assert [c for c in SEG if c["isolated"] and _field(c, "rowsum") == mode], mode
        assert [c for c in SEG if c["seg_only"] and c["Dp"] == 0 and _field(c, "rowsum") == mode], mode
    assert [c for c in SEG if not c["new_p"]] and [c for c in SEG if c["T"] == 0 and not c["seg_only"]]
    assert [c for c in SEG if set(c["need"]) == {"obj", "h"}]
    # embedding: one, two and many chunks; grid.y 1 and > 1; several tables; a table without a gradient; bad indices
    rules = [tuple(int(v) for v in re.findall(r"=(\d+)", k)) for c in EMB for k in c["kernels"].split(" | ") if k.startswith("chunk")]
    assert {r[1] for r in rules} >= {1, 2, 106} and {r[2] == 1 for r in rules} == {True, False}
    assert {r[0] for r in rules} >= {32, 64, 256, 1024}
    assert [c for c in EMB if len(c["tables"]) == 4 and len({t[1] for t in c["tables"]}) > 1]
    assert [c for c in EMB if c["need"] == (False, True)] and [c for c in EMB if c["oob"]]
    assert [c for c in EMB if c["tables"] == ((179, 128),)]
    assert {c["shape"] for c in RUN if c["family"] == "mask"} == {(5, 13, 3), (1, 1025, 1)}
    assert {c["image_id"] for c in RUN if c["family"] == "mask"} == {0, 2}
    (layer,) = LAYER
    assert (layer["Din"], layer["Dp"], layer["H"], layer["O"], layer["T"]) == (32, 32, 64, 12, 40)
    assert layer["graph"] == "padded" and layer["zero_conf"] is not None
    for c in CASES:                                                   # nothing near 2^31 elements
        assert c["B"] * max(c["T"], 1) * (2 * c["H"] + c["Dp"]) < 2 ** 27, c["name"]


def test_restated_rules_match_the_library():
    """csg_embed_bwd_workspace, csg_segment_avg_fwd_workspace and csg_gather_concat_bwd_workspace are functions of the chunk
    count and of rowsum_nseg, csg_graph_csr_lds of the builder choice: the restatements must give their values."""
    from canonicalsg2im_amd import _lib
    for rows in (1, 31, 32, 33, 1024, 1025, 27000):
        for n, dim in ((8, 8), (179, 128), (4, 256), (8, 32), (300, 12), (9, 9)):
            r = gc.emb_rule(rows, n, dim)
            want = r["chunks"] * n * dim * 4 if r["chunks"] > 1 else 0
            assert _lib.lib.csg_embed_bwd_workspace(rows, n, dim) == want, (rows, n, dim)
    pairs = {(c["O"], c["T"]) for c in CASES if c["family"] in ("csr", "seg", "layer")} | {
        (O, T) for O in (1, 253, 254, 255, 256, 1024, 1025) for T in (0, 1, 511, 512, 513, 65534, 65535, 65536, 70000)} | {
        (O, T) for O in (200, 254) for T in range(43500, 62000, 500)}
    for O, T in sorted(pairs):                              # the builder choice, from the function the dispatch itself asks
        lds = _lib.lib.csg_graph_csr_lds(T, O)
        want = {"refuse": -1, "plain": 0, "sorted": gc.csr_sorted_lds(T, O)}[gc.csr_builder(O, T)]
        assert lds == want, (O, T, lds, want)
    shapes = [(c["B"], c["O"], c["T"], c["H"], c["Din"]) for c in SEG] + [(2, 8, T, 32, 16) for T in range(185, 200)] + [
        (2, 1024, 30000, 8, 8), (1, 1, 24, 4, 4), (1, 1, 25, 4, 4)]
    for B, O, T, H, Din in shapes:
        ns = gc.rowsum_nseg(O, T)
        assert _lib.lib.csg_segment_avg_fwd_workspace(B, O, T, H) == (B * ns * (H + 1) * 4 + B * O * 8 if ns else 0), (B, O, T, H)
        assert _lib.lib.csg_gather_concat_bwd_workspace(B, O, T, Din) == (B * ns * Din * 4 + B * O * 8 if ns else 0), (B, O, T, Din)


def test_ref64_reproduces_the_reference_layer():
    """tests/golden/gconv.npz was written by the reference's own GraphTripleConv (float32): `layer_ref` in float64 gives its
    outputs, input gradients and every stored parameter gradient to 1e-6 of each tensor's largest entry."""
    meta, a = load_golden("gconv")
    H, Dp = meta["hidden"], meta["dp_out"]
    sd = {k[3:]: v.double().requires_grad_(True) for k, v in a.items() if k.startswith("sd:")}
    obj, pred = a["obj"].double().requires_grad_(True), a["pred"].double().requires_grad_(True)
    tr = torch.stack([a["edges"][..., 0], a["p"], a["edges"][..., 1]], -1)
    new_obj, new_p = gc.layer_ref(sd, obj, pred, tr, a["tt"], a["p"] != 0, H, Dp)
    ((new_obj * a["wo"].double()).sum() + (new_p * a["wp"].double()).sum()).backward()
    got = dict(new_obj=new_obj.detach(), new_p=new_p.detach(), gobj=obj.grad, gpred=pred.grad)
    got.update({"grad:" + k: v.grad for k, v in sd.items()})
    stored = [k for k in a if k.startswith("grad:")]
    assert set(stored) == {"grad:" + k for k in sd} and len(stored) == 9
    for k in ["new_obj", "new_p", "gobj", "gpred"] + stored:
        ref = a[k].double()
        err, scale = float((got[k] - ref).abs().max()), float(ref.abs().max())
        assert scale > 0 and err <= 1e-6 * scale, "%s: %.3e of scale %.3e" % (k, err, scale)


@pytest.mark.parametrize("c", CSR, ids=case_ids(CSR))
def test_host_csr_two_ways(c):
    d = gc.make_data(c)
    rp, col = gc.csr_host(d["tr"], c["O"])
    rp2, col2 = gc.csr_argsort(d["tr"], c["O"])
    assert torch.equal(rp, rp2) and torch.equal(col, col2)
    assert tuple(rp.shape) == (c["B"], c["O"] + 1) and tuple(col.shape) == (c["B"], max(2 * c["T"], 1))
    ids = torch.cat([d["tr"][..., 0], d["tr"][..., 2]], 1)
    bad = ((ids < 0) | (ids >= c["O"])).sum(1)
    assert torch.equal(rp[:, -1].long(), 2 * c["T"] - bad)
    if c["bad"]:                                          # both kinds of bad id, in both roles, in every image: entries dropped
        for col_ in (0, 2):
            assert bool((d["tr"][..., col_] == -1).any(1).all()) and bool((d["tr"][..., col_] == c["O"]).any(1).all())
        assert bool((rp[:, -1] < 2 * c["T"]).all())
    else:
        assert int(bad.sum()) == 0


def test_rows_are_what_they_say():
    for c in SEG + LAYER:
        d = gc.make_data(c)
        tr, valid, conf = d["tr"], d["valid"], d["conf"]
        lens = gc.row_lengths(tr, c["O"])
        assert bool(((tr[..., [0, 2]] >= 0) & (tr[..., [0, 2]] < max(c["O"], 1))).all()), c["name"]     # gather reads obj[id]
        assert bool((d["h"] >= 0).all()) and (c["T"] == 0 or 0.3 < float((d["h"] == 0).double().mean()) < 0.7), c["name"]
        assert set(d["tt"].flatten().tolist()) <= {0, 1, 2, 3}
        if c["T"]:
            assert bool(((conf == 0) & valid).any()) and bool(((conf == 1) & valid).any() or c["graph"] == "padded"), c["name"]
            assert bool(((conf > 0) & (conf < 1)).any()), c["name"]
        if c["expect"] is not None:                       # star / padded rows: the claimed hub, recounted
            dense = gc.rowsum_nseg(c["O"], c["T"]) > 0
            hub = int(lens.max())
            assert (gc.cdiv(hub, 128) if dense else hub) == c["expect"], (c["name"], hub)
            assert _field(c, "maxS" if dense else "maxrow") == str(c["expect"]), c["name"]
        if c["graph"] == "star":
            assert bool((tr[..., 0] == 0).all()) and bool((lens[:, 1:] > 0).all()), c["name"]
        if c["graph"] == "padded":
            keep = valid.sum(1).tolist()
            assert keep[0] == c["T"] and keep[-1] == 0 and keep == sorted(keep, reverse=True) and len(set(keep)) == c["B"]
            assert bool((tr[~valid] == 0).all()) and bool((conf[~valid] == 1).all()), c["name"]
            assert int(lens[-1, 0]) == 2 * c["T"]                                   # the all-padding image: one hub row
        if c["graph"] == "closure":
            assert c["T"] == c["O"] * (c["O"] - 1) and bool((lens == 2 * (c["O"] - 1)).all())
        if c["zero_conf"] is not None:
            z = ((tr[..., 0] == c["zero_conf"]) | (tr[..., 2] == c["zero_conf"])) & valid
            assert bool(z.any(1)[valid.any(1)].all()) and bool((conf[z] == 0).all()), c["name"]
            ref = gc.graph_ref64(c, d) if c["family"] == "seg" else None
            if ref is not None:                           # count 0 with valid edges: no division, pooled = the zero sum
                assert float(ref["pooled"][:, c["zero_conf"]].abs().max()) == 0.0
        for i in c["isolated"]:
            assert int(lens[:, i].sum()) == 0, c["name"]
        if c["family"] == "seg" and c["relu"] and c["T"] and "h" in c["need"]:
            ref = gc.graph_ref64(c, d)
            assert float(ref["dh"][d["h"] == 0].abs().max()) == 0.0 and float(ref["dh"].abs().max()) > 0
    for c in EMB:
        d = gc.make_data(c)
        for k, (n, _) in enumerate(c["tables"]):
            i = d["idx"][..., k].flatten()
            bad = (i < 0) | (i >= n)
            assert int(bad.sum()) == (2 if c["oob"] and k == 0 else 0)
            assert n > 64 or set(i[~bad].tolist()) == set(range(n)), c["name"]     # every table row is named
        if c["oob"]:
            ref = gc.graph_ref64(c, d)
            nan_rows = torch.isnan(ref["out"]).any(-1).flatten()
            assert int(nan_rows.sum()) == 2 and bool(torch.isfinite(ref["dtable_0"]).all())
            i = d["idx"][..., 0].flatten()
            assert set(i[nan_rows].tolist()) == {-1, c["tables"][0][0]}
    for c in RUN:
        if c["family"] == "mask":
            v = gc.make_data(c)["objs"][..., 0]
            assert bool((v == 0).any()) == (v.numel() > 1) and (bool((v == c["image_id"]).any()) or v.numel() == 1)


def test_layer_row_keeps_clear_of_every_relu_kink():
    """No pre-activation of net1's last layer (nor of the layer's other three ReLUs) lies within 1e-5 of that tensor's
    largest magnitude of zero, by the float64 reference alone: float32 and float64 take the same ReLU decisions."""
    (c,) = LAYER
    margins = gc.relu_margin(c, gc.make_data(c))
    assert set(margins) == {"net1.0", "net1.2", "net2.0", "net2.2"}
    for k, m in margins.items():
        assert m > 1e-5, "%s: a pre-activation at %.2e of the largest; move the row's seed" % (k, m)


def test_no_reads_from_outside_the_repository():
    """Neither the table nor the device test names a file outside the repository (the reference tree least of all): no
    absolute path literal, no parent-directory walk, no environment variable but the report's."""
    for mod in (gc, __import__("test_gpu_graph_paths")):
        src = inspect.getsource(mod)
        assert not re.search(r"""["'](/|~|\.\./)[A-Za-z_.]""", src), mod.__name__
        assert set(re.findall(r"environ[^\n]*?[\"']([A-Z_]+)[\"']", src)) <= {"GRAPH_PATHS_REPORT"}, mod.__name__
    assert os.path.dirname(os.path.abspath(gc.__file__)) == os.path.dirname(os.path.abspath(__file__))
