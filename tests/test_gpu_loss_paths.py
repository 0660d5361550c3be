"""Every spectral-norm, loss and resampling kernel path through the entry point the model uses (`ops.spectral_weight`,
`ops.spectral_weights`, `ops.l1_mean`, `GANLoss('hinge')`, `ops.maxpool2`, `ops.avgpool2`, `ops.upsample2x`,
`ops.avgpool3s2`, `ops.pool_fanout`, `ops.nearest_resize`) on a real MI355X, against the float64 restatement of each
contract (tests/loss_cases.py: the table and `ref64`).

Per row: the allocator's free blocks are filled with NaN before each run, so an element a kernel never writes shows up as
NaN; every output and every requested gradient must be finite (NaN rows: NaN exactly where the reference is) and of the
expected shape and memory format (W_eff channels-last exactly when the restated rule says so, maps NHWC), a gradient not
asked for must be None, a padded prediction buffer's pad channels must get exactly zero gradient, and a second run must
reproduce every tensor bit for bit — W_eff, u, v, sigma, gradients and losses: every reduction is an ordered sum.

Gates (loss_cases.rule).  exact: pure selections and copies — max-pool forward and backward, upsample2x and
nearest_resize forward, pool_fanout's full-resolution output.  gate, everything else: max error <= 1e-5 of the fp64
tensor's largest entry plus a 1e-6 floor (the gate of the conv plans and the geometry).  band: the spectral backward
subtracts c u v^T from the cotangent and the eps row divides by a sigma of 1e-23, so no fixed fraction can be derived for
those tensors; they are held against the float32 CPU evaluation of the same function on the same inputs, hip_err <=
max(3 x fp32_cpu_err, 1e-5 x scale) + 1e-6 (3: fp64_band.Band's factor).  scalar: the L1 and hinge values, 1e-5 relative
plus 1e-7.  On the hinge margin itself (rows hinge_tie_*) the gradient must be a subgradient: between 0 and the
off-margin gradient.  The measured pairs of every row are in profiles/loss_paths_gpu.txt."""
import os
import sys
import time

import pytest
import torch

import loss_cases as lc
from loss_cases import CASES, case_ids
from test_gpu_conv_plans import _nan_fill

pytestmark = pytest.mark.gpu
GATE, FLOOR, BAND, SCALAR_REL, SCALAR_ABS = 1e-5, 1e-6, 3.0, 1e-5, 1e-7
REPORT = os.environ.get("LOSS_PATHS_REPORT")          # a file that receives the table too (profiles/loss_paths_gpu.txt)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import ops as o
    return o


HEADER = """tests/test_gpu_loss_paths.py on an MI355X (gfx950): one line per row and tensor - the kernels and launch rules the row
reaches (*cap: the grid is capped and the stride loop goes round again), the largest fp64 entry (scale), the HIP error and
the float32 CPU evaluation's error on the same inputs, both as fractions of the scale, and the rule the tensor is held to:
exact = bit for bit; gate = 1e-5 of the scale + 1e-6; band = max(3 x fp32 CPU error, 1e-5 of the scale) + 1e-6 (spectral
backward, the eps row); scalar = 1e-5 relative + 1e-7.  Written by the test itself when LOSS_PATHS_REPORT names a file.
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


def _dev(t):
    return t.to(torch.float32).cuda()


def _leaf(t, grad):
    return t.detach().requires_grad_(bool(grad))


def _keep(t):
    return None if t is None else t.detach().cpu().clone()


# ------------------------------------------------------------------------------------------------- spectral
def _cotangent(shape, cot, g):
    """The logical (Cout, Cin, KH, KW) cotangent `g` in the row's memory layout."""
    if cot == "ohwi":
        t = g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    elif cot == "ohiw":
        t = g.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    elif cot == "padslice":
        Cout, Cin, KH, KW, K = lc.sn_dims(shape)
        buf = torch.full((Cout, KH, KW, lc.cdiv(Cin, 4) * 4 + 4), float("nan"), device="cuda")
        buf[..., :Cin] = g.permute(0, 2, 3, 1)
        t = buf[..., :Cin].permute(0, 3, 1, 2)
    elif cot == "colmajor":
        t = g.t().contiguous().t()
    else:
        t = g.contiguous()
    want = lc.cot_strides(shape, cot)
    assert all(s == w for s, w, n in zip(t.stride(), want, t.shape) if n > 1), (shape, cot, t.stride(), want)
    return t


def _run_spectral(ops, c, d):
    single = c["entry"] == lc.SW
    rows = [c] if single else [lc.BY_NAME[m] for m in c["members"]]
    data = [d] if single else d["members"]
    n = len(rows)
    grad = [single or r["name"] not in c["nograd"] for r in rows]
    back = [i for i, r in enumerate(rows) if grad[i] and r["name"] not in c["skip_bwd"]]
    ws = [_leaf(_dev(x["w"]), grad[i]) for i, x in enumerate(data)]
    us, vs = [_dev(x["u"]) for x in data], [_dev(x["v"]) for x in data]
    pre = (lambda i, k: k) if single else (lambda i, k: "m%02d.%s" % (i, k))
    res = {}

    def call(iterate, tag):
        outs = [ops.spectral_weight(ws[0], us[0], vs[0], iterate)] if single else ops.spectral_weights(list(zip(ws, us, vs)), iterate)
        for i, o in enumerate(outs):
            shape = rows[i]["shape"]
            Cout, Cin, KH, KW, K = lc.sn_dims(shape)
            if lc.sn_channels_last(shape):
                assert o.stride() == (K, 1, KW * Cin, Cin), "%s: W_eff is not channels-last" % rows[i]["name"]
            else:
                assert o.is_contiguous(), "%s: W_eff is not in the weight's own order" % rows[i]["name"]
            saved = o.grad_fn.saved_tensors                # (the n weights, then sigma | u_used | v_used of each)
            sigma = saved[n + i][:1]
            res[pre(i, "weff" + tag)], res[pre(i, "sigma" + tag)] = _keep(o), _keep(sigma)
            if iterate:
                res[pre(i, "u" + tag)], res[pre(i, "v" + tag)] = _keep(us[i]), _keep(vs[i])
        return outs

    def backward(outs, which, tag):
        if c["refuse"]:                                    # (single rows only: the backward must refuse)
            with pytest.raises(RuntimeError, match=c["refuse"]):
                outs[0].backward(_cotangent(c["shape"], c["cot"], _dev(d["cots"][which])))
        else:
            torch.autograd.backward([outs[i] for i in back],
                                    [_cotangent(rows[i]["shape"], rows[i]["cot"], _dev(data[i]["cots"][which])) for i in back])
        for i in range(n):
            res[pre(i, tag)] = _keep(ws[i].grad)
            ws[i].grad = None

    for k in (1, 2, 3):
        outs = call(True, str(k))
    backward(outs, 0, "dw3")
    before = [(u.clone(), v.clone()) for u, v in zip(us, vs)]
    outs = call(False, "_e")
    for i, (u, v) in enumerate(before):
        assert torch.equal(u, us[i]) and torch.equal(v, vs[i]), "%s: an eval call moved u / v" % rows[i]["name"]
    backward(outs, 1, "dw_e")
    return res


# ------------------------------------------------------------------------------------------------- losses
def _l1_operands(ops, c, d):
    a, b = _dev(d["a"]), _dev(d["b"])
    if c["fmt"] == "nhwc":
        a, b = ops.nhwc(a), ops.nhwc(b)
    elif c["fmt"] == "mixed":
        b = ops.nhwc(b)
    elif c["fmt"] == "sliced":                             # every second column of maps twice as wide: same strides, not dense
        a, b = (torch.cat([t, t], 3)[..., ::2] for t in (a, b))
    return _leaf(a, c["need"]), b.detach()


def _run_l1(ops, c, d):
    a, b = _l1_operands(ops, c, d)
    loss = ops.l1_mean(a, b)
    if c["need"]:
        (loss * c["gout"]).backward()
        assert a.grad.stride() == a.stride(), "%s: da is not in a's memory format" % c["name"]
    return dict(loss=_keep(loss), **({"da": _keep(a.grad)} if c["need"] else {}))


def _run_hinge(ops, c, d):
    from canonicalsg2im_amd.spade.models.networks.loss import GANLoss
    leaves, preds = [], []
    for x, pad, (s, f) in zip(d["xs"], d["pads"], c["maps"]):
        if f == "pad":                                     # channel 0 of a (B, h, w, 4) buffer: element stride 4
            leaf = _leaf(torch.cat([_dev(x), _dev(pad)], 1).permute(0, 2, 3, 1).contiguous(), c["need"])
            preds.append(leaf.permute(0, 3, 1, 2)[:, :1])
        else:
            leaf = _leaf(_dev(x), c["need"])
            preds.append(leaf)
        leaves.append(leaf)
    assert (ops.hinge_mean([p.detach() for p in preds], c["kind"]) is None) == (not lc.hinge_fused(c)), c["name"]
    real, for_d = {0: (True, False), 1: (True, True), 2: (False, True)}[c["kind"]]
    loss = GANLoss("hinge")([[p] for p in preds], real, for_discriminator=for_d)
    res = dict(loss=_keep(loss))
    if c["need"]:
        (loss * c["gout"]).sum().backward()
        for i, (leaf, (s, f)) in enumerate(zip(leaves, c["maps"])):
            g = leaf.grad
            if f == "pad":
                assert float(g[..., 1:].abs().max()) == 0.0, "%s: a pad channel of map %d got a gradient" % (c["name"], i)
                g = g.permute(0, 3, 1, 2)[:, :1]
            res["dx%d" % i] = _keep(g)
    return res


# ------------------------------------------------------------------------------------------------- resampling
def _is_nhwc(t):
    return t.permute(0, 2, 3, 1).is_contiguous()


def _resample_call(ops, c, x):
    e = c["entry"]
    if e == "nearest_resize":
        return [ops.nearest_resize(x, c["out_size"])]
    if e == "pool_fanout":
        return list(ops.pool_fanout(x))
    return [getattr(ops, e)(x)]


def _run_resample(ops, c, d):
    x = _leaf(ops.nhwc(_dev(d["x"])), c["need"])
    outs = _resample_call(ops, c, x)
    assert all(_is_nhwc(o) for o in outs), "%s: an output is not NHWC" % c["name"]
    res = {"out%d" % i: _keep(o) for i, o in enumerate(outs)}
    res["dx"] = None
    if c["need"]:
        used = lc._used(c)
        torch.autograd.backward([outs[i] for i in used], [ops.nhwc(_dev(d["douts"][i])) for i in used])
        assert _is_nhwc(x.grad), "%s: dx is not NHWC" % c["name"]
        res["dx"] = _keep(x.grad)
    return res


def _run(ops, c, d):
    if c["family"] == "spectral":
        return _run_spectral(ops, c, d)
    if c["entry"] == lc.L1:
        return _run_l1(ops, c, d)
    if c["entry"] == lc.HG:
        return _run_hinge(ops, c, d)
    return _run_resample(ops, c, d)


def _refused(ops, c, d):
    """A row whose forward must raise before any launch."""
    with pytest.raises(RuntimeError, match=c["refuse"]):
        if c["family"] == "spectral":
            ops.spectral_weight(_leaf(_dev(d["w"]), True), _dev(d["u"]), _dev(d["v"]), True)
        elif c["entry"] == lc.L1:
            ops.l1_mean(*_l1_operands(ops, c, d))
        else:
            _resample_call(ops, c, _leaf(_dev(d["x"]), True))


# ------------------------------------------------------------------------------------------------- judgement
def _judge(c, name, got, ref, fp32, tie=None):
    g = got.double()
    assert tuple(g.shape) == tuple(ref.shape), "%s %s: shape %s, expected %s" % (c["name"], name, tuple(g.shape), tuple(ref.shape))
    nan = torch.isnan(ref)
    assert bool(nan.any()) == (c["data"] == "nan" and name in ("loss", "out0")), (c["name"], name)
    assert torch.equal(torch.isnan(g), nan), "%s %s: NaN where the reference has none, or none where it has one%s" % (
        c["name"], name, " (got %r, expected %r)" % (float(g), float(ref)) if g.numel() == 1 else "")
    bad = int((~torch.isfinite(g[~nan])).sum())
    assert bad == 0, "%s %s: %d non-finite entries (memory no kernel wrote?)" % (c["name"], name, bad)
    rule = lc.rule(c, name)
    keep = ~nan if tie is None else ~nan & ~tie            # (the margin's own entries are judged as subgradients, below)
    scale = float(ref[~nan].abs().max()) if ref[~nan].numel() else 0.0
    err = float((g - ref)[keep].abs().max()) if ref[keep].numel() else 0.0
    ferr = float((fp32.double() - ref)[keep].abs().max()) if ref[keep].numel() else 0.0
    allow = {"exact": 0.0, "gate": GATE * scale + FLOOR, "band": max(BAND * ferr, GATE * scale) + FLOOR,
             "scalar": SCALAR_REL * scale + SCALAR_ABS}[rule]
    _say("| %-34s | %-10s | %-52s | scale %.2e | hip %.2e | fp32 cpu %.2e | %s |" % (
        c["name"], name, lc.describe(c)[:52], scale, err / max(scale, 1e-300), ferr / max(scale, 1e-300), rule))
    msgs = [] if err <= allow else ["%s %s: max error %.3e, allowed %.3e (%s; scale %.3e, fp32 cpu error %.3e)" % (
        c["name"], name, err, allow, rule, scale, ferr)]
    if tie is not None and bool(tie.any()):
        off = float(ref[~tie][ref[~tie] != 0][0])          # the off-margin gradient of this map: one value
        lo, hi = min(0.0, off), max(0.0, off)
        inside = bool(((g[tie] >= lo) & (g[tie] <= hi)).all())
        if not inside:
            msgs.append("%s %s: a gradient on the margin is outside [0, 1] x %.3e" % (c["name"], name, off))
    return msgs


@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_path_against_fp64(ops, c):
    t0 = time.time()
    d = lc.make_data(c)
    if c["refuse"] and c["refuse_at"] == "fwd":
        _refused(ops, c, d)
        return
    runs = []
    for _ in range(2):
        _nan_fill()
        runs.append(_run(ops, c, d))
        torch.cuda.synchronize()
    ref = lc.ref64(c, d)
    fp32 = lc.evaluate(c, d, torch.float32)
    assert set(ref) == set(runs[0]), sorted(set(ref) ^ set(runs[0]))
    failures = []
    for name, r in ref.items():
        got = runs[0][name]
        if r is None:
            assert got is None, "%s: %s was not asked for and came back" % (c["name"], name)
            continue
        assert got is not None, "%s: %s was asked for and did not come back" % (c["name"], name)
        tie = None
        if c["data"] == "tie" and name.startswith("dx"):
            tie = d["xs"][int(name[2:])] == lc.HINGE_CENTRE[c["kind"]]
        failures += _judge(c, name, got, r, fp32[name], tie)
        same = torch.equal(torch.nan_to_num(got, nan=123.0), torch.nan_to_num(runs[1][name], nan=123.0))
        assert same, "%s %s: a second run differs (max %.3e)" % (c["name"], name, float((got - runs[1][name]).abs().max()))
    _say("| %-34s | time       | %.2f s |" % (c["name"], time.time() - t0), report=False)
    assert not failures, "\n".join(failures)
