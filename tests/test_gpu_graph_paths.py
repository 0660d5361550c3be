"""Every scene-graph encoder kernel path through the entry point the model uses (`ops.graph_csr`, `ops.gather_concat`,
`ops.segment_avg`, `ops.embed`, `ops.real_object_mask`, and `GraphTripleConv` itself) on a real MI355X, against the float64
restatement of the contract (tests/graph_cases.py: the table and `graph_ref64`).

Per row: the allocator's free blocks are filled with NaN before each run, so a row, a partial or a gradient no kernel
writes shows up as NaN; every output and every requested gradient must be finite and of the expected shape, a gradient not
asked for must be None, and a second run must reproduce every tensor bit for bit (csrc/graph.hip: fixed summation order).

Bit-exact: the CSR arrays (row_ptr, and col up to row_ptr[O]), `cat`, the embedding forward, `dpred`, the masks.  `new_p`
must be float32(h) * float32(conf), correctly rounded.  Exactly zero: the subject and object slices of dh of an invalid
triplet (its predicate slice is dnew_p * conf like any other: the collate gives padding type 0, confidence 1), every dh
entry of a confidence-0 triplet, with h_is_relu every dh entry where h == 0, and pooled of an object whose summed
confidence is 0.

Gates.  `pooled` and the layer row's outputs: max error <= 1e-5 of the fp64 tensor's largest entry plus a 1e-6 floor (the
gate of the conv and geometry suites).  The summed gradients (dobj, dconf, dh, dtable, the layer's input and parameter
gradients) add up to 8 400 terms and dconf cancels a dot product against dcnt, so no fixed fraction can be derived for
them: they are held against the float32 CPU evaluation of the same restatement on the same inputs, hip_err <=
max(3 x fp32_cpu_err, 1e-5 x scale) + 1e-6 (3: fp64_band.Band's factor for "within the reference arithmetic's own noise").
The measured pairs of every row are in profiles/graph_paths_gpu.txt."""
import os
import sys
import time

import pytest
import torch

import graph_cases as gc
from graph_cases import CASES, case_ids
from test_gpu_conv_plans import _nan_fill

pytestmark = pytest.mark.gpu
GATE, FLOOR, BAND = 1e-5, 1e-6, 3.0
GATED = ("pooled", "new_obj", "new_p")
EXACT = ("row_ptr", "col", "cat", "out", "dpred", "mask")
REPORT = os.environ.get("GRAPH_PATHS_REPORT")         # a file that receives the table too (profiles/graph_paths_gpu.txt)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import ops as o
    return o


HEADER = """tests/test_gpu_graph_paths.py on an MI355X (gfx950): one line per row and tensor - the kernels the launch rules give the
row, the largest fp64 entry (scale), the HIP error and the float32 CPU restatement's error on the same inputs, both as
fractions of the scale, and the rule the tensor is held to: exact = bit for bit; rounded = bit for bit float32(h) *
float32(conf), the line shows that product's one rounding; gate = 1e-5 of the scale + 1e-6; band = max(3 x fp32 error, 1e-5
of the scale) + 1e-6 (the summed gradients).  Written by the test itself when GRAPH_PATHS_REPORT names a file.
"""
_report = []          # the open report file, once per session


def _say(line, report=True):
    print(line, file=sys.stderr)
    if REPORT and report:
        if not _report:
            _report.append(open(REPORT, "w"))
            _report[0].write(HEADER + "\n")
        _report[0].write(line + "\n")
        _report[0].flush()


def _dev(t, grad=False):
    return t.to(torch.float32).cuda().requires_grad_(grad)


def _layer(c, d):
    from canonicalsg2im_amd.sg2im.graph import GraphTripleConv, get_predicates_weights
    m = GraphTripleConv(c["Din"], c["Din"], c["Dp"], c["Dp"], c["H"], 1,
                        predicates_transitive_weights=get_predicates_weights(gc.P, "uniform"))
    m.load_state_dict({k: v.to(torch.float32) for k, v in d["sd"].items()})
    return m.cuda()


def _run(ops, c, d):
    """One forward (+ backward) of row `c`: {tensor name: device tensor or None}, named like graph_cases.graph_ref64."""
    f = c["family"]
    if f == "mask":
        return dict(mask=ops.real_object_mask(d["objs"].cuda(), c["image_id"]))
    if f == "csr":
        rp, col = ops.graph_csr(d["tr"].cuda(), c["O"])
        return dict(row_ptr=rp, col=col)
    if f == "embed":
        tabs = [_dev(t, need) for t, need in zip(d["tables"], c["need"])]
        out = ops.embed(d["idx"].cuda(), tabs)
        if any(c["need"]):
            out.backward(_dev(d["dout"]))
        return dict({"dtable_%d" % k: t.grad for k, t in enumerate(tabs)}, out=out)
    tr, valid = d["tr"].cuda(), d["valid"].to(torch.uint8).cuda()
    if f == "layer":
        m = _layer(c, d)
        obj, pred = _dev(d["obj"], True), _dev(d["pred"], True)
        new_obj, new_p = m(obj, pred, tr[..., [0, 2]].contiguous(), d["valid"].cuda(), d["tt"].cuda(), tr[..., 1].contiguous())
        torch.autograd.backward([new_obj, new_p], [_dev(d["dnew_obj"]), _dev(d["dnew_p"])])
        params = dict(m.named_parameters())
        res = dict(new_obj=new_obj, new_p=new_p, dobj=obj.grad, dpred=pred.grad, dw_trans=params["predicates_transitive_weights"].grad)
        res.update({"d" + k: params[k].grad for k in gc.LAYER_PARAMS})
        return res
    need = c["need"]
    rp, col = ops.graph_csr(tr, c["O"])
    res = dict(cat=None, dobj=None, dpred=None)
    if not c["seg_only"]:
        obj, pred = _dev(d["obj"], "obj" in need), _dev(d["pred"], "pred" in need)
        cat = ops.gather_concat(obj, pred, tr, rp, col)
        cat.backward(_dev(d["dcat"]))
        res.update(cat=cat, dobj=obj.grad, dpred=pred.grad)
    h, conf = _dev(d["h"], "h" in need), _dev(d["conf"], "conf" in need)
    pooled, new_p = ops.segment_avg(h, conf, valid, tr, rp, col, c["H"], c["Dp"], h_is_relu=c["relu"])
    if c["new_p"]:
        torch.autograd.backward([pooled, new_p], [_dev(d["dpooled"]), _dev(d["dnew_p"])])
    else:
        pooled.backward(_dev(d["dpooled"]))
    res.update(pooled=pooled, new_p=new_p, dh=h.grad, dconf=conf.grad)
    return res


def _rule(c, name):
    """exact: bit for bit; rounded: new_p of a seg row, held to float32(h) * float32(conf) bit for bit by _seg_properties (its
    distance from fp64, one rounding, is reported under the gate); gate; band."""
    if c["family"] == "layer":
        return "gate" if name in GATED else "band"
    if name == "new_p":
        return "rounded"
    if name in EXACT:
        return "exact"
    return "gate" if name in GATED else "band"


def _judge(c, name, got, ref, fp32, skip=None):
    """None, or what is wrong with tensor `name`.  `skip`: a boolean mask of entries left out of the comparison (the two
    NaN rows of the out-of-range embedding row, which are checked to BE NaN instead)."""
    assert tuple(got.shape) == tuple(ref.shape), "%s %s: shape %s, expected %s" % (c["name"], name, tuple(got.shape), tuple(ref.shape))
    rule = _rule(c, name)
    if skip is not None:
        assert bool(torch.isnan(got[skip]).all()) and bool(torch.isnan(ref[skip]).all()), "%s %s: a bad index must read NaN" % (c["name"], name)
        got, ref, fp32 = got[~skip], ref[~skip], fp32[~skip]
    if not got.is_floating_point():
        assert torch.equal(got, ref.to(got.dtype)), "%s %s: not bit-exact" % (c["name"], name)
        _say("| %-28s | %-14s | %-78s | %d integers | exact |" % (c["name"], name, c["kernels"][:78], got.numel()))
        return None
    g = got.double()
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, "%s %s: %d non-finite entries (memory no kernel wrote?)" % (c["name"], name, bad)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((g - ref).abs().max()) if ref.numel() else 0.0
    ferr = float((fp32.double() - ref).abs().max()) if ref.numel() else 0.0
    allow = {"exact": 0.0, "rounded": GATE * scale + FLOOR, "gate": GATE * scale + FLOOR,
             "band": max(BAND * ferr, GATE * scale) + FLOOR}[rule]
    _say("| %-28s | %-14s | %-78s | scale %.2e | hip %.2e | fp32 %.2e | %s |" % (
        c["name"], name, c["kernels"][:78], scale, err / max(scale, 1e-300), ferr / max(scale, 1e-300), rule))
    return None if err <= allow else "%s %s: max error %.3e, allowed %.3e (scale %.3e, fp32 error %.3e, %s)" % (
        c["name"], name, err, allow, scale, ferr, rule)


def _refuse(ops, c, d):
    if c["family"] == "csr":
        with pytest.raises(RuntimeError, match=c["refuse"]):
            ops.graph_csr(d["tr"].cuda(), c["O"])
    else:
        tabs = [_dev(t, True) for t in d["tables"]]
        with pytest.raises(RuntimeError, match=c["refuse"]):
            ops.embed(d["idx"].cuda(), tabs)
    torch.cuda.synchronize()


def _seg_properties(c, d, got):
    """What must hold bit for bit on a segment-average row."""
    H, Dp = c["H"], c["Dp"]
    h32, conf32 = d["h"].to(torch.float32), d["conf"].to(torch.float32)
    assert torch.equal(got["new_p"], h32[..., H:H + Dp] * conf32.unsqueeze(-1)), "%s: new_p is not float32(h) * float32(conf)" % c["name"]
    cnt = torch.zeros(c["B"], c["O"], dtype=torch.float64)
    for b in range(c["B"]):
        m = d["valid"][b]
        cnt[b] = cnt[b].index_add(0, d["tr"][b, m, 0], d["conf"][b, m]).index_add(0, d["tr"][b, m, 2], d["conf"][b, m])
    if bool((cnt == 0).any()):
        assert float(got["pooled"][cnt == 0].abs().max()) == 0.0, "%s: pooled of a count-0 object is not exactly 0" % c["name"]
    dh = got["dh"]
    if dh is None or not dh.numel():
        return
    off, zero = ~d["valid"], d["conf"] == 0
    if bool(off.any()):
        so = torch.cat([dh[..., :H], dh[..., H + Dp:]], -1)
        assert float(so[off].abs().max()) == 0.0, "%s: dh (subject / object slices) of an invalid triplet is not exactly 0" % c["name"]
    if bool(zero.any()):
        assert float(dh[zero].abs().max()) == 0.0, "%s: dh of a confidence-0 triplet is not exactly 0" % c["name"]
    if not c["new_p"] and Dp:
        assert float(dh[..., H:H + Dp].abs().max()) == 0.0, "%s: dh (predicate slice) without a new_p cotangent is not 0" % c["name"]
    if c["relu"]:
        assert float(dh[h32 == 0].abs().max()) == 0.0, "%s: h_is_relu left a gradient where h == 0" % c["name"]
    if c["graph"] == "padded":                        # the all-padding image: count 0, pooled 0, nothing flows to its objects
        assert float(got["pooled"][-1].abs().max()) == 0.0 and float(so[-1].abs().max()) == 0.0, c["name"]


@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_path_against_fp64(ops, c):
    t0 = time.time()
    d = gc.make_data(c)
    if c["refuse"]:
        _refuse(ops, c, d)
        return
    runs = []
    for _ in range(2):
        _nan_fill()
        o = _run(ops, c, d)
        torch.cuda.synchronize()
        runs.append({t: (None if v is None else v.detach().cpu().clone()) for t, v in o.items()})
    ref = gc.graph_ref64(c, d)
    fp32 = gc.graph_ref64(c, d, torch.float32)
    assert set(ref) == set(runs[0]), sorted(set(ref) ^ set(runs[0]))
    failures = []
    for name, r in ref.items():
        got = runs[0][name]
        if r is None:
            assert got is None, "%s: %s was not asked for and came back" % (c["name"], name)
            continue
        assert got is not None, "%s: %s was asked for and did not come back" % (c["name"], name)
        skip = None
        if name == "col":                             # entries past row_ptr[O] are not part of the contract
            n = ref["row_ptr"][:, -1].long()
            keep = torch.arange(r.shape[1]).unsqueeze(0) < n.unsqueeze(1)
            got, r = torch.where(keep, got, torch.zeros_like(got)), torch.where(keep, r, torch.zeros_like(r))
            assert torch.equal(runs[0]["row_ptr"][:, -1].long(), n), "%s: row_ptr[O]" % c["name"]
        if name == "out" and c["oob"]:                # the one exemption from "all finite": the two rows of the bad indices
            skip = torch.isnan(r)
            assert int(skip.any(-1).sum()) == 2 and bool((skip.any(-1, keepdim=True) == skip)[..., :c["tables"][0][1]].all())
        msg = _judge(c, name, got, r, fp32[name], skip)
        if msg:
            failures.append(msg)
        a, b = runs[0][name], runs[1][name]
        if name == "col":
            a, b = torch.where(keep, a, torch.zeros_like(a)), torch.where(keep, b, torch.zeros_like(b))
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), "%s %s: a second run differs" % (c["name"], name)
    if c["family"] == "seg":
        _seg_properties(c, d, runs[0])
        if c["T"] == 0:
            assert float(runs[0]["pooled"].abs().max()) == 0.0 and float(runs[0]["dobj"].abs().max()) == 0.0
            assert runs[0]["cat"].numel() == 0 and runs[0]["new_p"].numel() == 0
    _say("| %-28s | time   | %.2f s |" % (c["name"], time.time() - t0), report=False)
    assert not failures, "\n".join(failures)
