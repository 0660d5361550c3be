"""The spectral-norm / loss / resampling matrix on the CPU (tests/loss_cases.py): `ref64` against independent float64
evaluations (torch.nn.utils.spectral_norm on a float64 module, F.max_pool2d, F.avg_pool2d in both forms, F.interpolate,
F.l1_loss, the oracle's hinge), every row's distance from the discontinuities of its gradients, the float32 evaluation's
room under the device gate, and the table's coverage of every kernel branch, computed from the restated launch rules."""
import functools

import pytest
import torch
import torch.nn.functional as F

import loss_cases as lc
from loss_cases import CASES, case_ids

RUN = [c for c in CASES if not (c["refuse"] and c["refuse_at"] == "fwd")]
REQUIRED = """sn_64x32x3x3 sn_128x64x4x4 sn_64x512x3x3 sn_1x16x3x3 sn_33x8x3x3 sn_20x12x1x1 sn_16x6x4x4 sn_48x100 sn_2052x4x3x3
sn_2056x4096x1x1 sn_8x960x4x4 sn_8x1024x4x4 sn_refuse_k27 sn_eps sn_multi13 l1_n4 l1_nchw l1_nhwc l1_zeros
l1_stride_4x64x260x260 l1_gout l1_nan l1_refuse_strides l1_refuse_not_dense l1_refuse_n6 hinge_5scales_fallback
hinge_2ch_fallback hinge_nan_k0 hinge_nan_k1 hinge_nan_k2 hinge_tie_k1 hinge_tie_k2 avgpool3s2_2x36x9x9 avgpool3s2_2x36x8x10
avgpool3s2_1x4x1x1 avgpool3s2_1x4x2x1 fanout_both fanout_full fanout_pool upsample2x_2x8x5x7 upsample2x_stride_1x4x1026x1026
nearest_7_to_5 nearest_9x70_to_5x33 nearest_5_to_13 nearest_identity nearest_to_1x1 nearest_from_1x1 maxpool2_refuse_c6
maxpool2_refuse_h1 avgpool2_refuse_c6 avgpool2_refuse_h1""".split() + \
    ["hinge_k%d_s%d_%s" % (k, n, f) for k in (0, 1, 2) for n in (1, 2, 4) for f in ("pad", "contig")] + \
    ["%s_%s" % (p, r) for p in ("maxpool2", "avgpool2") for r in ("min_1x4x2x2", "odd_2x12x7x9", "even_2x12x6x8", "negative",
                                                                   "ties_zeros", "nan", "stride_1x4x2052x2052")]


@functools.lru_cache(maxsize=1)
def _row(name):
    """(data, ref64) of a row, built once for the checks that follow each other on it."""
    c = lc.BY_NAME[name]
    d = lc.make_data(c)
    return d, lc.ref64(c, d)


def _agree(c, ref, other, what, tol=1e-10):
    assert set(ref) == set(other), sorted(set(ref) ^ set(other))
    for name, r in ref.items():
        if r is None:
            assert other[name] is None, name
            continue
        o = other[name]
        assert o is not None and tuple(r.shape) == tuple(o.shape), (c["name"], name)
        nan = torch.isnan(r)
        assert torch.equal(nan, torch.isnan(o)), "%s %s vs %s: NaNs elsewhere" % (c["name"], name, what)
        assert bool(nan.any()) == (c["data"] == "nan"), (c["name"], name)
        r, o = r[~nan], o[~nan]
        scale = float(r.abs().max()) if r.numel() else 0.0
        err = float((r - o).abs().max()) if r.numel() else 0.0
        assert err <= tol * scale + 1e-300, "%s %s vs %s: %.3e of scale %.3e" % (c["name"], name, what, err, scale)


# ------------------------------------------------------------------------------------------------- independent evaluations
def _torch_spectral(c, d, need_w=True, skip_bwd=False):
    """torch.nn.utils.spectral_norm on a float64 module, its pre-forward hook called by hand."""
    shape = c["shape"]
    m = (torch.nn.Linear(shape[1], shape[0], bias=False) if len(shape) == 2 else
         torch.nn.Conv2d(shape[1], shape[0], shape[2:], bias=False)).double()
    m = torch.nn.utils.spectral_norm(m, eps=lc.SN_EPS)
    with torch.no_grad():
        m.weight_orig.copy_(d["w"])
        m.weight_u.copy_(d["u"])
        m.weight_v.copy_(d["v"])
    hook = next(iter(m._forward_pre_hooks.values()))
    back = need_w and not skip_bwd and not c["refuse"]
    res = {}

    def grad(cot):
        if not back:
            return None
        m.weight_orig.grad = None
        m.weight.backward(cot)
        return m.weight_orig.grad.clone()

    m.train()
    for k in (1, 2, 3):
        hook(m, None)
        u, v = m.weight_u.detach().clone(), m.weight_v.detach().clone()
        sigma = torch.dot(u, m.weight_orig.detach().reshape(shape[0], -1) @ v)
        res.update({"weff%d" % k: m.weight.detach().clone(), "u%d" % k: u, "v%d" % k: v, "sigma%d" % k: sigma.reshape(1)})
    res["dw3"] = grad(d["cots"][0])
    m.eval()
    hook(m, None)
    assert torch.equal(m.weight_u, u) and torch.equal(m.weight_v, v)
    res.update(weff_e=m.weight.detach().clone(), sigma_e=sigma.reshape(1))
    res["dw_e"] = grad(d["cots"][1])
    return res


def _independent(c, d):
    if c["family"] == "spectral":
        if c["entry"] == lc.SW:
            return _torch_spectral(c, d)
        res = {}
        for i, (m, dm) in enumerate(zip(c["members"], d["members"])):
            r = _torch_spectral(dict(lc.BY_NAME[m], refuse=None), dm, m not in c["nograd"], m in c["skip_bwd"])
            res.update({"m%02d.%s" % (i, k): t for k, t in r.items()})
        return res
    if c["entry"] == lc.L1:
        a = d["a"].clone().requires_grad_(bool(c["need"]))
        loss = F.l1_loss(a, d["b"])
        res = dict(loss=loss.detach())
        if c["need"]:
            (loss * c["gout"]).backward()
            res["da"] = a.grad
        return res
    if c["entry"] == lc.HG:
        import oracle.functional as of
        xs = [x.clone().requires_grad_(bool(c["need"])) for x in d["xs"]]
        real, for_d = {0: (True, False), 1: (True, True), 2: (False, True)}[c["kind"]]
        loss = of.gan_loss_multiscale([[x] for x in xs], real, for_d)
        res = dict(loss=loss.detach().reshape(1))
        if c["need"]:
            (loss * c["gout"]).backward()
            res.update({"dx%d" % i: x.grad for i, x in enumerate(xs)})
        return res
    x = d["x"].clone().requires_grad_(bool(c["need"]))
    e = c["entry"]
    pool3 = lambda t: F.avg_pool2d(t, 3, 2, 1, count_include_pad=False)
    outs = {"maxpool2": lambda: [F.max_pool2d(x, 2, 2)], "avgpool2": lambda: [F.avg_pool2d(x, 2, 2)],
            "upsample2x": lambda: [F.interpolate(x, scale_factor=2, mode="nearest")],
            "nearest_resize": lambda: [F.interpolate(x, size=c["out_size"], mode="nearest")],
            "avgpool3s2": lambda: [pool3(x)], "pool_fanout": lambda: [x * 1, pool3(x)]}[e]()
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    res["dx"] = None
    if c["need"]:
        sum((outs[i] * d["douts"][i]).sum() for i in lc._used(c)).backward()
        res["dx"] = x.grad
    return res


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_row_on_the_cpu(c):
    """One row, its data and reference built once: `ref64` against the independent float64 evaluation, outputs and every
    requested gradient to 1e-10 of each tensor's scale; the row's distance from its discontinuities; the float32
    evaluation's room under the device gate."""
    d, ref = _row(c["name"])
    _agree(c, ref, _independent(c, d), "torch")
    _keeps_clear_of_discontinuities(c, d)
    if c["data"] != "nan":
        _float32_leaves_room_under_the_gate(c, d, ref)


NEAREST = [c for c in RUN if c["entry"] == "nearest_resize"]


@pytest.mark.parametrize("c", NEAREST, ids=case_ids(NEAREST))
def test_nearest_index_rule_is_atens(c):
    """The source index is part of the contract and lives in ATen's float32 arithmetic: the restatement on float32 data
    against F.interpolate, bit for bit."""
    d, _ = _row(c["name"])
    mine = lc.evaluate(dict(c, need=()), d, torch.float32)["out0"]
    assert torch.equal(mine, F.interpolate(d["x"].float(), size=c["out_size"], mode="nearest"))


def test_a_float64_scale_would_pick_other_pixels():
    """Why the index is float32: row nearest_14x6_to_46x74 reads other pixels along both axes under a float64 scale."""
    import numpy as np
    c = lc.BY_NAME["nearest_14x6_to_46x74"]
    for n_in, n_out in zip(c["shape"][2:], c["out_size"]):
        f64 = np.minimum(np.floor(np.arange(n_out) * (n_in / n_out)).astype(np.int64), n_in - 1)
        assert int((torch.from_numpy(f64) != lc.nearest_index(n_out, n_in)).sum()) > 0, (n_in, n_out)


def _keeps_clear_of_discontinuities(c, d):
    """Judged on the reference alone.  (a) every hinge margin off the tie is more than 1e-3 from 0 (tie rows: exactly 0 or
    that far); (b) every L1 difference is exactly 0 or beyond 1e-4; (c) every max-pool window's winner ties bit for bit or
    leads by more than 1e-4.  A row that fails moves its seed."""
    if c["entry"] == lc.HG and c["kind"] != 0:
        m = lc.hinge_margins(c, d)
        on = m == 0
        assert bool(on.any()) == (c["data"] == "tie"), c["name"]
        assert float(m[~on].abs().min()) > 1e-3, c["name"]
        assert bool((m < 0).any() and (m > 0).any()), c["name"]           # the values straddle the margin
    if c["entry"] == lc.L1:
        diff = (d["a"] - d["b"]).abs()
        diff = diff[~torch.isnan(diff)]
        assert bool((diff == 0).any()) == (c["data"] == "zeros"), c["name"]
        assert float(diff[diff != 0].min()) > 1e-4, c["name"]
    if c["entry"] == "maxpool2":
        lead = lc.maxpool_leads(d["x"])
        assert float(lead.min()) > 1e-4, c["name"]
        ties = int((lc.windows2(d["x"]) == lc.windows2(d["x"]).max(-1, keepdim=True).values).sum(-1).gt(1).sum())
        assert ties > 0 or c["data"] != "ties", c["name"]


def _float32_leaves_room_under_the_gate(c, d, ref):
    """The device test holds the gated tensors to 1e-5 of the scale (scalars: 1e-5 relative).  A row whose float32 CPU
    evaluation is itself beyond 7e-6 there would test the number format, not the kernel; the exact tensors are exact in
    float32 as well."""
    f32 = lc.evaluate(c, d, torch.float32)
    for name, r in ref.items():
        if r is None or not r.numel():
            continue
        rule = lc.rule(c, name)
        scale, err = float(r.abs().max()), float((f32[name].double() - r).abs().max())
        if rule == "exact":
            assert err == 0.0, (c["name"], name)
        elif rule == "scalar":
            assert err <= 7e-6 * scale + 1e-7, "%s %s: float32 is %.2e of the value off" % (c["name"], name, err / scale)
        elif rule == "gate":
            assert err <= 7e-6 * scale + 1e-6, "%s %s: float32 is %.2e of the scale off" % (c["name"], name, err / scale)


def test_eps_row_clamps_both_norms_and_stays_normal():
    """sn_eps: ||W^T u|| and ||W v|| are under eps = 1e-12 on every training-mode call, so both clamps act, and every
    quantity the kernels form — products included — is a normal float32 number (no flush to zero decides the row)."""
    c = lc.BY_NAME["sn_eps"]
    d, ref = _row(c["name"])
    W2, u, v = d["w"].reshape(64, -1), d["u"], d["v"]
    seen = [W2]
    for _ in range(3):
        t = W2.t() @ u
        seen += [t, W2 * u.view(-1, 1)]
        assert float(t.norm()) < lc.SN_EPS
        v = t / lc.SN_EPS
        s = W2 @ v
        seen += [v, s, W2 * v.view(1, -1)]
        assert float(s.norm()) < lc.SN_EPS
        u = s / lc.SN_EPS
        seen += [u, u * s, torch.dot(u, s).reshape(1)]
    sigma = torch.dot(u, s)
    for g in d["cots"]:
        cc = (g.reshape(64, -1) * W2).sum() / sigma
        seen += [g.reshape(64, -1) * W2, cc.reshape(1), cc * u, torch.outer(cc * u, v)]
    seen += [r for r in ref.values() if r is not None]
    tiny, huge = float(torch.finfo(torch.float32).tiny), float(torch.finfo(torch.float32).max)
    for t in seen:
        a = t.abs()
        assert float(a[a > 0].min()) > 4 * tiny and float(a.max()) < huge / 4


def _rows(cases=RUN, **kw):
    return [c for c in cases if all((v(c[k]) if callable(v) else c[k] == v) for k, v in kw.items())]


def test_table_covers_every_kernel_branch_and_corner():
    names = case_ids()
    assert len(set(names)) == len(names)
    missing = [n for n in REQUIRED if n not in lc.BY_NAME]
    assert not missing, "rows deleted from the table: %s" % missing
    sn = _rows(CASES, entry=lc.SW)
    runs = [c for c in sn if not (c["refuse"] and c["refuse_at"] == "fwd")]
    dims = {c["name"]: lc.sn_dims(c["shape"]) for c in sn}
    # ---- R regimes: 1; Cout (< 32); the cap of 32 with and without empty chunks, with a short last chunk; 512 // blocks
    R = {c["name"]: lc.sn_R(dims[c["name"]][0], dims[c["name"]][4]) for c in runs}
    empty = {c["name"]: lc.sn_empty_chunks(dims[c["name"]][0], dims[c["name"]][4]) for c in runs}
    assert R["sn_1x16x3x3"] == 1 and R["sn_20x12x1x1"] == 20 and R["sn_64x512x3x3"] == 32 and R["sn_8x960x4x4"] == 8
    assert R["sn_33x8x3x3"] == 32 and empty["sn_33x8x3x3"] == 15 and empty["sn_64x32x3x3"] == 0
    assert [n for n in R if R[n] == 32 and empty[n] == 0 and dims[n][0] % 32]             # a last chunk that is not full
    assert [n for n in R if R[n] == 512 // lc.cdiv(dims[n][4], 1024) < min(32, dims[n][0]) and empty[n] > 0]
    # ---- column blocks of 1024: exactly one, several, a ragged last one
    assert dims["sn_128x64x4x4"][4] == 1024 and dims["sn_64x512x3x3"][4] == 4608
    assert [n for n in dims if dims[n][4] < 1024] and [n for n in dims if dims[n][4] > 1024 and dims[n][4] % 1024]
    # ---- both d_sn_scale paths, each with and without the capped loop; the transpose buffer's limit; the plain fallbacks
    rules = {c["name"]: lc.sn_scale_rule(c["shape"]) for c in runs}
    for path in ("cl", "plain"):
        for capped in (False, True):
            assert [n for n, r in rules.items() if r["path"] == path and r["capped"] == capped], (path, capped)
    assert rules["sn_2052x4x3x3"] == dict(path="cl", grid=2048, capped=True, lds=9 * 8 * 4)
    assert rules["sn_2056x4096x1x1"]["path"] == "plain" and 2056 * 4096 // 4 == 2105344 > 2048 * 1024
    assert rules["sn_8x960x4x4"] == dict(path="cl", grid=8, capped=False, lds=61696) and 61696 <= lc.SN_T_BYTES
    assert rules["sn_8x1024x4x4"]["path"] == "plain" and 16 * 1028 * 4 > lc.SN_T_BYTES
    assert rules["sn_20x12x1x1"]["path"] == "plain" and rules["sn_16x6x4x4"]["path"] == "plain" and 6 % 4
    assert rules["sn_48x100"]["path"] == "plain" and rules["sn_64x32x3x3"]["path"] == "cl"
    assert all(r["lds"] <= lc.SN_T_BYTES for r in rules.values())
    # ---- the backward's LDS row: exactly at the limit, and refused beyond it; K % 4
    assert dims["sn_8x960x4x4"][4] == lc.SN_BWD_MAXK
    over = [c for c in sn if c["refuse_at"] == "bwd"]
    assert over and all(c["refuse"] and dims[c["name"]][4] > lc.SN_BWD_MAXK and dims[c["name"]][4] % 4 == 0 for c in over)
    assert all(dims[c["name"]][4] <= lc.SN_BWD_MAXK for c in runs if not c["refuse"])
    assert [c for c in sn if c["refuse"] and c["refuse_at"] == "fwd" and dims[c["name"]][4] % 4]
    # ---- every cotangent layout; which of them are dense permutations and which go through .contiguous()
    assert {c["cot"] for c in runs if not c["refuse"]} == set(lc.COTS)
    for c in runs:
        Cout, Cin, KH, KW, K = dims[c["name"]]
        dense = lc.rows_dense(lc.cot_strides(c["shape"], c["cot"]), (Cin, KH, KW), K)
        assert dense == (c["cot"] in ("contig", "ohwi", "ohiw")), c["name"]
        assert lc.cot_goes_through_contiguous(c["shape"], c["cot"]) == (c["cot"] in ("padslice", "colmajor")), c["name"]
    assert [c for c in runs if c["cot"] == "ohiw" and c["shape"][2] > 1 and c["shape"][1] > 1]   # not OHWI, not contiguous
    assert [c for c in sn if len(c["shape"]) == 2] and [c for c in sn if c["shape"][0] == 1]
    assert lc.BY_NAME["sn_eps"]["scale"] == 1e-14 and lc.BY_NAME["sn_eps"]["shape"] == (64, 32, 3, 3)
    # ---- the multi-tensor form: 13 = 12 + 1, every early return taken, a weight without grad, an output left out
    multi = lc.BY_NAME["sn_multi13"]
    mem = [lc.BY_NAME[m] for m in multi["members"]]
    assert len(mem) == lc.SN_MAXT + 1 and len(set(multi["members"])) == 13 and all(m["entry"] == lc.SW for m in mem)
    assert set(multi["members"]) <= set(REQUIRED)
    first, last = mem[:lc.SN_MAXT], mem[lc.SN_MAXT]
    md = [lc.sn_dims(m["shape"]) for m in first]
    assert lc.sn_dims(last["shape"])[0] * lc.sn_dims(last["shape"])[4] < 1024
    assert len({d_[0] for d_ in md}) > 1 and len({lc.cdiv(d_[4], 1024) for d_ in md}) > 1       # g_row, g_part_x from the largest
    assert len({lc.sn_R(d_[0], d_[4]) for d_ in md}) > 1                                          # g_part_y
    assert len({lc.sn_scale_rule(m["shape"])["grid"] for m in first}) > 1                         # g_scale
    assert len(multi["nograd"]) == 1 and len(multi["skip_bwd"]) == 1 and set(multi["nograd"]) | set(multi["skip_bwd"]) <= set(multi["members"])
    assert all(m["name"] in multi["skip_bwd"] for m in mem if m["refuse"])
    assert {m["cot"] for m in mem} >= {"contig", "ohwi", "ohiw", "padslice"}
    # ---- ew_grid: capped and uncapped for every elementwise kernel, forward and backward
    seen = {}
    for c in RUN:
        for k, n in lc.launches(c):
            seen.setdefault(k, set()).add(lc.ew_capped(n))
            assert lc.ew_grid(n) == min(max(-(-n // 256), 1), 4096)
    kernels = ["l1_partial", "l1_bwd", "hinge_bwd"] + [p + s for p in ("maxpool2", "avgpool2", "upsample2x", "avgpool3s2", "nearest")
                                                        for s in ("_fwd", "_bwd")]
    assert sorted(seen) == sorted(kernels)
    for k in kernels:
        assert seen[k] == {False, True}, (k, seen[k])
    assert 4 * 64 * 260 * 260 > 16777216 and 1026 * 1026 == 1052676 > 1048576
    # ---- L1: layouts, the zero block, the upstream gradient, NaN, the three refusals
    l1 = _rows(CASES, entry=lc.L1)
    assert {c["fmt"] for c in l1} >= {"nchw", "nhwc", "mixed", "sliced"} and [c for c in l1 if c["gout"] != 1.0]
    assert len([c for c in l1 if c["refuse"]]) == 3 and [c for c in l1 if c["data"] == "nan"] and [c for c in l1 if c["data"] == "zeros"]
    # ---- hinge: kinds x 1, 2, 4 scales x padded / contiguous; the map sizes; the fallbacks; NaN for every kind; ties
    hg = _rows(CASES, entry=lc.HG)
    fused = [c for c in hg if lc.hinge_fused(c)]
    for kind in (0, 1, 2):
        for n in (1, 2, 4):
            for f in ("pad", "contig"):
                assert [c for c in fused if c["kind"] == kind and len(c["maps"]) == n and all(m[1] == f for m in c["maps"])
                        and c["data"] == "randn"], (kind, n, f)
        assert [c for c in fused if c["kind"] == kind and c["data"] == "nan"], kind
    assert {m[0] for c in fused for m in c["maps"]} >= {(1, 1, 3, 5), (16, 1, 35, 35), (3, 1, 19, 23)}
    assert {c["kind"] for c in fused if c["data"] == "tie"} == {1, 2}
    assert [c for c in hg if len(c["maps"]) == 5] and [c for c in hg if any(m[0][1] == 2 for m in c["maps"])]
    assert not [c for c in hg if not lc.hinge_fused(c) and len(c["maps"]) <= 4 and all(m[0][1] == 1 for m in c["maps"])]
    # ---- resampling corners
    for e in ("maxpool2", "avgpool2"):
        rs = _rows(RUN, entry=e)
        assert {c["shape"] for c in rs} >= {(1, 4, 2, 2), (2, 12, 7, 9), (2, 12, 6, 8), (1, 4, 2052, 2052)}
        assert {c["data"] for c in rs} >= {"randn", "neg", "ties", "nan"}
        assert len([c for c in _rows(CASES, entry=e) if c["refuse"]]) == 2
    assert {c["shape"] for c in _rows(RUN, entry="avgpool3s2")} >= {(2, 36, 9, 9), (2, 36, 8, 10), (1, 4, 1, 1), (1, 4, 2, 1)}
    assert {c["mode"] for c in _rows(RUN, entry="pool_fanout")} == {"both", "full", "pool"}
    nr = _rows(RUN, entry="nearest_resize")
    assert {(c["shape"][2:], c["out_size"]) for c in nr} >= {((7, 7), (5, 5)), ((9, 70), (5, 33)), ((5, 5), (13, 13)), ((6, 7), (6, 7)),
                                                             ((7, 9), (1, 1)), ((1, 1), (4, 6))}
    neg = lc.make_data(lc.BY_NAME["maxpool2_negative"])["x"]
    assert float(neg.max()) < 0
    # ---- nothing near 2^31 elements
    for c in RUN:
        shapes = [c["shape"]] if c["shape"] else [m[0] for m in c["maps"] or []]
        assert all(torch.Size(s).numel() < 2 ** 27 for s in shapes), c["name"]


def test_restated_rules_match_the_library():
    """sn_R through csg_spectral_norm_workspace, and the L1 partial-sum grid through csg_l1_mean_workspace (the library
    loads without a device)."""
    from canonicalsg2im_amd import _lib
    from canonicalsg2im_amd.ops import _rows_dense
    for c in _rows(CASES, entry=lc.SW):
        Cout, Cin, KH, KW, K = lc.sn_dims(c["shape"])
        want = -1 if K % 4 else max((lc.sn_R(Cout, K) * K + K + Cout) * 4, Cout * 8)
        assert _lib.lib.csg_spectral_norm_workspace(Cout, K) == want, c["name"]
        st = lc.cot_strides(c["shape"], c["cot"])
        assert _rows_dense(st, (Cin, KH, KW), K) == lc.rows_dense(st, (Cin, KH, KW), K)
    for c in _rows(RUN, entry=lc.L1):
        n = torch.Size(c["shape"]).numel()
        assert _lib.lib.csg_l1_mean_workspace(n) == lc.ew_grid(lc.cdiv(n // 4, 4)) * 8, c["name"]
