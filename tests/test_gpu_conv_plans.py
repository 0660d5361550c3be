"""Every convolution plan through the entry points the model uses (`ops.conv2d` / `ops.linear`) on a real MI355X, against
the float64 restatement of the contract (tests/conv_cases.py: the table and `conv2d_ref64`).

Per row: the plan that actually served the call (`ops.plan_conv` as `_Conv2d.forward` calls it) must be the row's; y and
every gradient that was asked for must be within 1e-5 of the tensor's largest fp64 entry (plus a 1e-6 floor: the
acceptance gate of F(4x4,3x3), tests/test_gpu_wino4.py), and a gradient not asked for must come back None.  The
allocator's free blocks are filled with NaN before each run, so an output edge, channel slice or workspace a kernel never
writes shows up as NaN.  Every row runs twice and must reproduce its outputs bit for bit (README: every reduction is an
ordered sum).  One row per weight-gradient family also writes its gradient into a registered destination slot."""
import sys
import time

import pytest
import torch
import torch.nn.functional as F

from conv_cases import ACTS, CASES, LEAKY, case_ids, kink_mask, make_data, reference
from test_conv_plan import _code

pytestmark = pytest.mark.gpu
GATE, FLOOR = 1e-5, 1e-6
SLICE = 4                     # a "slice" operand: channels [4, 4 + C) of a tensor with 8 more


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import ops as o
    return o


def _nan_fill():
    """Hand the caching allocator ~1.4 GB of NaN-filled blocks of both pools (<= 1 MB: small, larger: large): what the
    next run allocates and does not write reads NaN."""
    torch.cuda.synchronize()
    held = []
    for nbytes, count in ((4 << 10, 64), (64 << 10, 64), (512 << 10, 32), (2 << 20, 32), (16 << 20, 16), (128 << 20, 8)):
        held.extend(torch.full((nbytes // 4,), float("nan"), device="cuda") for _ in range(count))
    torch.cuda.synchronize()
    del held


def _place(t, fmt, grad):
    """(leaf, operand): the operand in memory format `fmt` on the device; gradients land on the leaf."""
    t = t.cuda()
    if fmt == "cl":
        t = t.contiguous(memory_format=torch.channels_last)
    elif fmt == "slice":
        pad = torch.full((t.shape[0], SLICE) + tuple(t.shape[2:]), 0.5, device=t.device)
        leaf = torch.cat([pad, t, pad], 1).contiguous(memory_format=torch.channels_last).requires_grad_(grad)
        return leaf, leaf[:, SLICE:SLICE + t.shape[1]]
    leaf = t.requires_grad_(grad)
    return leaf, leaf


def _grad(leaf):
    return None if leaf is None or leaf.grad is None else leaf.grad


def _run(ops, c, d, packs, slot=False):
    """One forward + backward of row `c`: {tensor name: device tensor or None}."""
    act, slope = ACTS[c["act"]]
    need = c["need"]
    if c["pair"]:
        s, k1 = c["in_act"], c["pair"]["k"]
        w1 = d["w1"].cuda().requires_grad_(True)
        b1 = d["b1"].cuda().requires_grad_(True)
        wl, wv = _place(d["w"], c["wfmt"], True)
        b = d["b"].cuda().requires_grad_(True) if c["bias"] else None
        if c["linear"]:
            B, cin1 = c["B"], c["pair"]["Cin"]
            xl = d["x"].reshape(3, B // 3, cin1).cuda().requires_grad_(True)
            y1 = ops.linear(xl, w1.view(c["Cin"], cin1), b1, LEAKY, s, grad_is_pre=True)
            y = ops.linear(y1, wv.view(c["Cout"], c["Cin"]), b, in_act=(LEAKY, s))
            y.backward(d["dy"].reshape(3, B // 3, c["Cout"]).cuda())
            y1, y = y1.reshape(B, -1, 1, 1), y.reshape(B, -1, 1, 1)
            dx = xl.grad.reshape(B, cin1, 1, 1)
        else:
            xl, xv = _place(d["x"], c["xfmt"], True)
            y1 = ops.conv2d(xv, w1, b1, 1, k1 // 2, LEAKY, s, grad_is_pre=True)
            y = ops.conv2d(y1, wv, b, c["s"], c["p"], act, slope, in_act=(LEAKY, s))
            y.backward(d["dy"].cuda())
            dx = xl.grad
        return dict(y1=y1, y=y, dx=dx, dw1=w1.grad, db1=b1.grad, dw=_grad(wl), db=_grad(b))
    xl, xv = _place(d["x"], c["xfmt"], "x" in need)
    wl, wv = _place(d["w"], c["wfmt"], "w" in need)
    b = d["b"].cuda().requires_grad_("b" in need) if c["bias"] else None
    res = d["res"].cuda().requires_grad_("r" in need) if c["res"] else None
    if slot:
        dest = torch.full((wv.numel(),), float("nan"), device="cuda")
        ops.set_grad_destinations({(wv.data_ptr(), wv.numel()): dest})
    try:
        y = ops.conv2d(xv, wv, b, c["s"], c["p"], act, slope, residual=res, packs=packs, dx_range=c["dx_range"],
                       in_act=None if c["in_act"] is None else (LEAKY, c["in_act"]), pre_slope=c["pre_slope"])
        if y.requires_grad:
            y.backward(d["dy"].cuda())
    finally:
        if slot:
            ops.clear_grad_destinations()
    out = dict(y=y, dx=_grad(xl), dw=_grad(wl), db=_grad(b), dres=_grad(res))
    if slot:            # the slot mirrors the channels-last weight's memory: [Cout][KH][KW][Cin]
        Cout, Cin, k = c["Cout"], c["Cin"], c["k"]
        out["slot"] = dest.view(Cout, k, k, Cin).permute(0, 3, 1, 2)
    return out


def _expect(c, ref):
    """The reference laid out like what the leaves receive: a slice operand's gradient sits inside zeros."""
    ref = dict(ref)
    for t, fmt in (("dx", c["xfmt"]), ("dw", c["wfmt"])):
        if fmt == "slice" and ref.get(t) is not None:
            ref[t] = F.pad(ref[t], (0, 0, 0, 0, SLICE, SLICE))
    return ref


def _judge(c, t, got, ref, plan):
    g = got.detach().double().cpu()
    assert tuple(g.shape) == tuple(ref.shape), "%s %s: shape %s, expected %s" % (c["name"], t, tuple(g.shape), tuple(ref.shape))
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, "%s %s: %d non-finite entries (memory no kernel wrote?)" % (c["name"], t, bad)
    scale = float(ref.abs().max())
    err = float((g - ref).abs().max())
    print("| %-22s | %-5s | %-38s | %.2e | %.0e |" % (c["name"], t, plan, err / max(scale, 1e-300), GATE), file=sys.stderr)
    assert err <= GATE * scale + FLOOR, "%s %s (%s): max error %.3e, scale %.3e, gate %.0e of the scale" % (
        c["name"], t, plan, err, scale, GATE)


@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_plan_against_fp64(ops, c, monkeypatch):
    t0 = time.time()
    for k, v in c["knobs"].items():
        monkeypatch.setattr(ops, k, v)
    d = make_data(c)
    packs = ops.pack_conv_weight(d["w"].cuda()) if c["packs"] else None
    if c["refuse"]:
        _, xv = _place(d["x"], c["xfmt"], "x" in c["need"])
        _, wv = _place(d["w"], c["wfmt"], "w" in c["need"])
        with pytest.raises(RuntimeError, match=c["refuse"]):
            ops.conv2d(xv, wv, d["b"].cuda(), c["s"], c["p"], *ACTS[c["act"]], packs=packs)
        return

    real, calls = ops.plan_conv, []

    def recorder(*a, **k):
        p = real(*a, **k)
        if sys._getframe(1).f_code is ops._Conv2d.forward.__code__:        # not conv2d's few-output probe
            calls.append(_code(p))
        return p

    monkeypatch.setattr(ops, "plan_conv", recorder)
    want = list(c["plan"]) if c["pair"] else [c["plan"]]
    ref = None if c["pair"] else reference(c, d)[0]            # (masks the incoming gradient at the row's kinks)
    runs = []
    for _ in range(2):
        _nan_fill()
        del calls[:]
        o = _run(ops, c, d, packs)
        torch.cuda.synchronize()
        assert calls == want, "%s: served by %s, expected %s" % (c["name"], calls, want)
        runs.append({t: (None if v is None else v.detach().cpu().clone()) for t, v in o.items()})
    if c["pair"]:
        # the consumer's gate reads the producer's output: where its fp64 pre-activation lies within rounding of the
        # kink, either side is right — the reference takes the side the device's output took there
        ref, pre1 = reference(c, d)
        near = kink_mask(pre1) == 0
        if bool(near.any()):
            ref, _ = reference(c, d, gate_x=torch.where(near, runs[0]["y1"].double(), ref["y1"]))
    ref = _expect(c, ref)
    plan = " / ".join(want)
    for t, r in ref.items():
        got = runs[0][t]
        if r is None:
            assert got is None, "%s: %s was not asked for and came back" % (c["name"], t)
            continue
        assert got is not None, "%s: %s was asked for and did not come back" % (c["name"], t)
        _judge(c, t, got, r, plan)
        assert torch.equal(got, runs[1][t]), "%s %s: a second run differs (max %.3e)" % (
            c["name"], t, float((got - runs[1][t]).abs().max()))
    if c["slot"]:
        _nan_fill()
        o = _run(ops, c, d, packs, slot=True)
        torch.cuda.synchronize()
        _judge(c, "slot", o["slot"], ref["dw"], plan)
        assert torch.equal(o["slot"].cpu(), runs[0]["dw"]), "%s: the slot differs from the gradient without one" % c["name"]
    print("| %-22s | time  | %.2f s |" % (c["name"], time.time() - t0), file=sys.stderr)
