"""The convolution plan matrix of tests/test_gpu_conv_plans.py, on the CPU: every row's plan is what `ops.plan_conv` returns
for it, the rows cover every kernel family the planner can name and every call option of `ops.conv2d`, and the float64
reference `conv2d_ref64` agrees with a separately written torch autograd composition of the same contract."""
import inspect
import re

import pytest
import torch
import torch.nn.functional as F

from conv_cases import CASES, LEAKY, NONE, TANH, conv2d_ref64, make_data, pair_plan_args, plan_args, reference, row
from test_conv_plan import _code


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import ops as o
    return o


def _plans(ops, c, monkeypatch):
    with monkeypatch.context() as m:
        for k, v in c["knobs"].items():
            m.setattr(ops, k, v)
        got = _code(ops.plan_conv(**plan_args(c)))
        return (_code(ops.plan_conv(**pair_plan_args(c))), got) if c["pair"] else got


def test_table_rows_keep_their_plans(ops, monkeypatch):
    got = {c["name"]: _plans(ops, c, monkeypatch) for c in CASES if not c["refuse"]}
    assert got == {c["name"]: c["plan"] for c in CASES if not c["refuse"]}


def _family(tok):
    return "wino" if tok in ("wino2", "wino4") else tok


def test_table_covers_the_planner_vocabulary(ops):
    """Each family literal plan_conv assigns to fwd / dx / wgrad is served by a row (both Winograd variants where there
    are two): a family added to the planner without a row fails here."""
    vocab = {"fwd": set(), "dx": set(), "wgrad": set()}
    for line in inspect.getsource(ops.plan_conv).splitlines():
        m = re.match(r"\s*(fwd|dx|wgrad)\b[\w, ]*=(.*)", line)
        if m:
            vocab[m.group(1)].update(re.findall(r'"(\w+)"', m.group(2)))
    assert vocab["fwd"] >= {"few", "wino", "wino34", "gemm", "direct"} and "colsum" in vocab["wgrad"], vocab
    seen = {"fwd": set(), "dx": set(), "wgrad": set()}
    for c in CASES:
        for code in ((c["plan"],) if isinstance(c["plan"], str) else (c["plan"] or ())):
            for key, tok in zip(("fwd", "dx", "wgrad"), code.split()):
                seen[key].add(tok)
    for key in vocab:
        assert vocab[key] <= {_family(t) for t in seen[key]}, (key, vocab[key] - {_family(t) for t in seen[key]})
    assert {"wino2", "wino4"} <= seen["fwd"] and {"wino2", "wino4"} <= seen["dx"]


def test_table_covers_every_call_option():
    def has(pred):
        return any(pred(c) for c in CASES)
    checks = {
        "act lrelu": lambda c: c["act"] == "lrelu", "act relu": lambda c: c["act"] == "relu",
        "act tanh": lambda c: c["act"] == "tanh", "no bias": lambda c: not c["bias"] and not c["pair"],
        "residual": lambda c: c["res"] and "r" in c["need"], "packs": lambda c: c["packs"] and not c["refuse"],
        "packs, padded Cin": lambda c: c["packs"] and c["Cin"] % 4 and not c["refuse"],
        "dx_range from 0": lambda c: c["dx_range"] and c["dx_range"][0] == 0,
        "dx_range above 0": lambda c: c["dx_range"] and c["dx_range"][0] > 0,
        "in_act ReLU": lambda c: c["in_act"] == 0.0, "in_act LeakyReLU": lambda c: c["in_act"] == 0.2,
        "grad_is_pre pair": lambda c: c["pair"] and not c["linear"], "linear pair": lambda c: c["linear"],
        "pre_slope in the loaders": lambda c: c["pre_slope"] is not None and c["Cin"] < 256,
        "pre_slope, Cin >= 256": lambda c: c["pre_slope"] is not None and c["Cin"] >= 256,
        "1 output": lambda c: c["Cout"] == 1, "3 outputs": lambda c: c["Cout"] == 3,
        "padded Cin / Cout": lambda c: c["Cin"] % 4 and c["Cout"] % 4,
        "only x": lambda c: c["need"] == "x" and not c["packs"], "only w": lambda c: c["need"] == "w",
        "only b": lambda c: c["need"] == "b", "nothing": lambda c: c["need"] == "",
        "knob": lambda c: c["knobs"], "refusal": lambda c: c["refuse"],
        "x channels-last": lambda c: c["xfmt"] == "cl", "x slice": lambda c: c["xfmt"] == "slice",
        "w channels-last": lambda c: c["wfmt"] == "cl", "w slice": lambda c: c["wfmt"] == "slice",
    }
    assert [k for k, pred in checks.items() if not has(pred)] == []
    slots = {c["plan"].split()[2] for c in CASES if c["slot"]}
    assert slots == {"gemm_tn", "wino4w", "wino", "direct"}
    assert all(c["wfmt"] == "cl" and "w" in c["need"] for c in CASES if c["slot"])


def test_in_act_rows_cover_every_gated_backward_data_family(ops):
    """in_act is served by: a Winograd launch with the gate in its epilogue and one split over the input channels (gate
    as a separate pass), F(3x3,4x4), the GEMM kernel, the direct kernel in one launch and over stride-2 parity classes
    (separate pass) — each by a single-convolution row and as the consumer of a grad_is_pre pair."""
    from canonicalsg2im_amd._lib import lib
    for pairs in (False, True):
        kinds = set()
        for c in CASES:
            if c["in_act"] is None or bool(c["pair"]) != pairs:
                continue
            dx = (c["plan"][1] if pairs else c["plan"]).split()[1]
            if dx in ("wino2", "wino4"):
                d = ops._wino_desc(c["B"], c["H"], c["W"], c["Cout"], c["Cin"])
                ws = (lib.csg_wino4_conv_workspace if dx == "wino4" else lib.csg_wino_conv_workspace)(d)
                kinds.add("wino split" if ws > 0 else "wino folded")
            elif dx == "direct":
                kinds.add("direct classes" if c["s"] > 1 else "direct one launch")
            else:
                kinds.add(dx)
        assert kinds == {"wino folded", "wino split", "wino34", "gemm", "direct one launch", "direct classes"}, (pairs, kinds)


def test_packs_need_a_frozen_weight_when_the_input_channels_are_padded(ops):
    w = torch.randn(8, 3, 3, 3, requires_grad=True)
    wp = F.pad(w.detach(), (0, 0, 0, 0, 0, 1))
    packs = ops.FrozenPacks(wp.permute(0, 2, 3, 1).contiguous(), wp.permute(1, 2, 3, 0).contiguous())
    with pytest.raises(RuntimeError, match="packs= needs a frozen weight"):
        ops.conv2d(torch.randn(1, 3, 6, 6), w, None, 1, 1, packs=packs)
    assert [c["name"] for c in CASES if c["refuse"]] == ["packs_trainable_padded"]


# ------------------------------------------------------------------------------------ the reference itself
def _leaky(t, s):
    """LeakyReLU as autograd's where / mul: slope s below and at 0, like the kernels' gate."""
    return torch.where(t > 0, t, t * s)


def _autograd64(x, w, b, stride, pad, act, slope, res, pre_slope, in_act, dx_range, dy, need):
    """The same contract composed from torch.nn.functional and differentiated by autograd: an in_act x is LeakyReLU(p) of
    a pre-activation p (p = x where x > 0, x / s below; the gradient is taken at p), dx_range lets the gradient through
    channels [lo, hi) only."""
    x, w, dy = x.double(), w.double(), dy.double()
    if in_act is not None:
        leaf = torch.where(x > 0, x, x / in_act if in_act > 0 else torch.zeros_like(x)).requires_grad_("x" in need)
        xx = _leaky(leaf, in_act)
        assert torch.equal(xx.detach(), x)
    else:
        leaf = x.clone().requires_grad_("x" in need)
        xx = leaf
    if dx_range is not None:
        m = torch.zeros(1, x.shape[1], 1, 1, dtype=torch.float64)
        m[:, dx_range[0]:dx_range[1]] = 1
        xx = xx * m + (xx * (1 - m)).detach()
    xin = _leaky(xx, pre_slope) if pre_slope is not None else xx
    wl = w.clone().requires_grad_("w" in need)
    bl = b.double().clone().requires_grad_("b" in need) if b is not None else None
    rl = res.double().clone().requires_grad_("r" in need) if res is not None else None
    pre = F.conv2d(xin, wl, bl, stride, pad)
    y = _leaky(pre, slope) if act == LEAKY else torch.tanh(pre) if act == TANH else pre
    if rl is not None:
        y = y + rl
    if y.requires_grad:
        y.backward(dy)
    g = lambda t: None if t is None else t.grad      # noqa: E731
    return dict(y=y.detach(), dx=g(leaf), dw=g(wl), db=g(bl), dres=g(rl))


REF_CASES = [
    # B, Cin, Cout, H, W, k, s, p, act, slope, bias, res, pre_slope, in_act, dx_range, need
    (2, 5, 6, 7, 9, 3, 1, 1, NONE, 0.0, True, True, None, None, None, "xwbr"),
    (2, 6, 8, 9, 9, 4, 2, 2, LEAKY, 0.2, True, False, None, None, None, "xwb"),
    (1, 4, 4, 6, 7, 3, 1, 1, LEAKY, 0.0, False, False, None, None, None, "xw"),
    (2, 8, 3, 8, 6, 3, 1, 1, TANH, 0.0, True, False, 0.2, None, None, "xwb"),
    (2, 8, 4, 7, 7, 3, 1, 1, NONE, 0.0, True, False, None, 0.0, None, "xwb"),
    (2, 8, 4, 9, 8, 4, 2, 2, NONE, 0.0, False, False, None, 0.2, None, "xw"),
    (2, 12, 8, 10, 10, 4, 2, 2, LEAKY, 0.2, True, False, None, None, (4, 8), "xwb"),
    (2, 8, 4, 6, 6, 3, 1, 1, NONE, 0.0, True, False, None, None, None, "w"),
    (2, 8, 4, 6, 6, 3, 1, 1, NONE, 0.0, True, False, None, None, None, "b"),
    (2, 8, 4, 6, 6, 1, 1, 0, NONE, 0.0, True, False, None, 0.0, None, "x"),
]


@pytest.mark.parametrize("case", REF_CASES)
def test_reference_matches_autograd(case):
    B, Cin, Cout, H, W, k, s, p, act, slope, bias, res, pre_slope, in_act, dx_range, need = case
    g = torch.Generator().manual_seed(B * 1000 + Cin * 10 + Cout)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    if in_act is not None:
        x = F.leaky_relu(x, in_act)
        x[:, :, ::3, ::2] = 0.0                                  # exact zeros: the gate is 1 above 0 only
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64) if bias else None
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    r = torch.randn(B, Cout, OH, OW, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(B, Cout, OH, OW, generator=g, dtype=torch.float64)
    got = conv2d_ref64(x, w, b, s, p, act, slope, r, pre_slope, in_act, dx_range, dy, need)
    want = _autograd64(x, w, b, s, p, act, slope, r, pre_slope, in_act, dx_range, dy, need)
    for t, v in want.items():
        if v is None:
            assert got[t] is None, t
        else:
            assert torch.allclose(got[t], v, rtol=1e-12, atol=1e-12), (t, float((got[t] - v).abs().max()))


def test_pair_reference_is_the_plain_chain():
    """A grad_is_pre -> in_act pair's expectations equal autograd through conv -> LeakyReLU -> conv."""
    c = row("pair", None, 2, 9, 9, 16, 8, 3, 2, 1, in_act=0.2, bias=True, pair=dict(Cin=8, k=3))
    d = make_data(c)
    ref, _ = reference(c, d)
    x, w1, b1, w, b = (d[t].double().requires_grad_(True) for t in ("x", "w1", "b1", "w", "b"))
    y1 = _leaky(F.conv2d(x, w1, b1, 1, 1), 0.2)
    y = F.conv2d(y1, w, b, 2, 1)
    y.backward(d["dy"].double())
    want = dict(y1=y1, y=y, dx=x.grad, dw1=w1.grad, db1=b1.grad, dw=w.grad, db=b.grad)
    for t, v in want.items():
        assert torch.allclose(ref[t], v.detach(), rtol=1e-12, atol=1e-12), t


def test_in_act_rows_read_exact_zeros():
    for c in CASES:
        if c["in_act"] is not None and not c["pair"]:
            x = make_data(c)["x"]
            assert bool((x == 0).any()) and bool((x < 0).any()) == (c["in_act"] > 0), c["name"]
