"""The convolution plan matrix: one row per kernel plan `ops.plan_conv` can return (and per call option of `ops.conv2d`),
with `conv2d_ref64`, a plain float64 CPU restatement of the contract `ops.conv2d` documents.  Used by
tests/test_gpu_conv_plans.py (each row through `ops.conv2d` / `ops.linear` on the device) and tests/test_conv_cases.py
(on the CPU: the table against the planner, the reference against torch autograd).

A row (dict, built by `row`) holds
  name, plan      — the id and the plan `test_conv_plan._code` prints for it ("fwd dx wgrad"; a tuple of two for a
                    producer -> consumer pair, producer first)
  B, H, W, Cin, Cout, k, s, p — batch, input size, channels, square kernel, stride, padding (Cout: the real count)
  act             — "none" | "relu" | "lrelu" (slope 0.2) | "tanh"
  bias, res       — bias / residual
  packs           — frozen weight through pack_conv_weight (the weight does not require grad)
  dx_range        — (lo, hi) or None
  in_act          — the producer's LeakyReLU slope (x is its output) or None
  pre_slope       — conv2d's pre_slope or None
  need            — which of "x", "w", "b" require grad ("r": the residual as well)
  xfmt, wfmt      — "nchw" (contiguous), "cl" (channels-last) or "slice" (a channel slice of a larger tensor)
  knobs           — ops module attributes to set for the row (non-default planner knobs)
  slot            — also run with a registered gradient destination (ops.set_grad_destinations) for the weight
  pair            — producer of a grad_is_pre / in_act pair: dict(Cin=, k=), LeakyReLU(in_act) + bias; the row's own
                    geometry is the consumer's
  linear          — run through ops.linear with x of shape (3, B // 3, Cin) (B, H, W = rows, 1, 1)
  refuse          — conv2d must refuse the call with a RuntimeError matching this pattern
"""
import zlib

import torch
import torch.nn.functional as F

LEAKY, NONE, TANH = 1, 0, 2
ACTS = {"none": (NONE, 0.0), "relu": (LEAKY, 0.0), "lrelu": (LEAKY, 0.2), "tanh": (TANH, 0.0)}


def row(name, plan, B, H, W, Cin, Cout, k, s, p, act="none", bias=False, res=False, packs=False, dx_range=None, in_act=None,
        pre_slope=None, need=None, xfmt="nchw", wfmt="nchw", knobs=None, slot=False, pair=None, linear=False, refuse=None):
    if need is None:
        need = "x" if packs else ("xwb" if bias else "xw")
    return dict(name=name, plan=plan, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p, act=act, bias=bias, res=res,
                packs=packs, dx_range=dx_range, in_act=in_act, pre_slope=pre_slope, need=need, xfmt=xfmt, wfmt=wfmt,
                knobs=knobs or {}, slot=slot, pair=pair, linear=linear, refuse=refuse)


CASES = [
    # ---- few-output kernels (csrc/fewn.hip)
    row("conv_img", "few few_direct few", 2, 40, 72, 64, 3, 3, 1, 1, act="tanh", bias=True, pre_slope=0.2),
    row("patch_head", "few few few", 2, 18, 18, 512, 1, 4, 1, 2, bias=True, xfmt="cl"),
    row("few_pre_slope_wide", "few few few", 2, 16, 16, 512, 3, 3, 1, 1, act="tanh", bias=True, pre_slope=0.2),
    row("few_bias_only", "few - few", 2, 18, 18, 512, 1, 4, 1, 2, bias=True, need="b"),
    # ---- Winograd F(2x2,3x3) / F(4x4,3x3) (csrc/wino.hip, csrc/wino4.hip) and their weight gradients
    row("wino2_lrelu", "wino2 wino2 wino4w", 4, 16, 16, 64, 64, 3, 1, 1, act="lrelu", bias=True, wfmt="cl", slot=True),
    row("wino2_residual", "wino2 wino2 wino4w", 4, 16, 16, 64, 64, 3, 1, 1, bias=True, res=True, need="xwbr", xfmt="cl"),
    row("wino2_dx_direct", "wino2 direct direct", 2, 24, 40, 48, 36, 3, 1, 1, bias=True),
    row("wino2_wgrad_f2", "wino2 wino2 wino", 2, 16, 32, 32, 32, 3, 1, 1, bias=True, wfmt="cl", slot=True),
    row("wino4", "wino4 wino4 wino4w", 4, 64, 64, 64, 320, 3, 1, 1, bias=True, wfmt="slice"),
    row("wino4_split_cin", "wino4 wino2 wino4w", 1, 32, 64, 256, 64, 3, 1, 1, xfmt="slice"),
    row("wino4_need_x", "wino4 wino4 -", 4, 64, 64, 64, 320, 3, 1, 1, bias=True, need="x"),
    row("wino4_need_w", "wino4 - wino4w", 4, 64, 64, 64, 320, 3, 1, 1, bias=True, need="w"),
    # ---- Winograd F(3x3,4x4) (csrc/wino4.hip) on the PatchGAN's 4x4 / stride 1 layers
    row("wino34_fwd_only", "wino34 - -", 1, 17, 17, 64, 64, 4, 1, 2, bias=True, need=""),
    row("wino34_colsum", "wino34 - colsum", 1, 17, 17, 64, 64, 4, 1, 2, bias=True, need="b"),
    row("wino34_dx_pad2", "direct wino34 direct", 1, 17, 17, 64, 64, 4, 1, 2, bias=True, act="lrelu"),
    row("wino34_dx_pad1", "direct wino34 direct", 2, 16, 19, 64, 64, 4, 1, 1, bias=True),
    row("wino34_fwd_mode3", "wino34 wino34 direct", 1, 17, 17, 64, 64, 4, 1, 2, bias=True, knobs={"WINO34_MODE": 3}),
    # ---- plain GEMM kernels (csrc/gemm.hip)
    row("gemm", "gemm gemm gemm_tn", 2, 128, 128, 256, 128, 1, 1, 0, bias=True, wfmt="cl", slot=True),
    # ---- the direct implicit-GEMM kernel (csrc/igemm.hip)
    row("direct_s2", "direct direct direct", 3, 33, 33, 36, 64, 4, 2, 2, act="lrelu", bias=True, wfmt="cl", slot=True),
    row("direct_1x1", "direct direct direct", 2, 9, 11, 8, 12, 1, 1, 0, bias=True, xfmt="slice", wfmt="slice"),
    row("direct_padded", "direct direct direct", 2, 8, 8, 3, 5, 3, 1, 1, bias=True),
    row("direct_residual", "direct direct direct", 2, 10, 10, 8, 16, 3, 1, 1, bias=True, res=True, need="xwbr"),
    row("range_lo0", "direct range direct", 2, 34, 34, 36, 64, 4, 2, 2, act="lrelu", bias=True, dx_range=(0, 32)),
    row("range_lo32", "direct range direct", 2, 34, 34, 36, 64, 4, 2, 2, act="lrelu", bias=True, dx_range=(32, 36),
        xfmt="cl"),
    # ---- frozen weights (pack_conv_weight), each run twice: the second call takes the cached operands
    row("packs_wino2", "wino2 wino2 -", 4, 16, 16, 64, 64, 3, 1, 1, act="relu", bias=True, packs=True),
    row("packs_wino4", "wino4 wino4 -", 4, 64, 64, 64, 320, 3, 1, 1, act="relu", bias=True, packs=True),
    row("packs_vgg_first", "direct direct -", 2, 12, 12, 3, 64, 3, 1, 1, act="relu", bias=True, packs=True),
    row("packs_trainable_padded", None, 2, 12, 12, 3, 64, 3, 1, 1, act="relu", bias=True, packs=True, need="xw",
        refuse="packs= needs a frozen weight"),
    # ---- in_act: x is a (Leaky)ReLU output, dx comes back multiplied by its derivative
    row("in_act_wino_folded", "wino2 wino2 wino4w", 4, 16, 16, 128, 64, 3, 1, 1, in_act=0.0),
    row("in_act_wino_split", "wino2 wino4 wino4w", 1, 32, 32, 64, 2048, 3, 1, 1, in_act=0.0),
    row("in_act_wino34", "direct wino34 direct", 2, 16, 19, 64, 64, 4, 1, 1, in_act=0.2),
    row("in_act_gemm", "gemm gemm gemm_tn", 2, 128, 128, 256, 128, 1, 1, 0, bias=True, in_act=0.0),
    row("in_act_direct", "direct direct direct", 2, 9, 9, 16, 8, 3, 1, 1, bias=True, in_act=0.2),
    row("in_act_direct_s2", "direct direct direct", 2, 17, 17, 12, 16, 4, 2, 2, bias=True, in_act=0.0),
    # ---- grad_is_pre producer -> in_act consumer pairs, one per gate-taking backward-data family of the consumer
    row("pair_wino_folded", ("wino2 wino2 wino", "wino2 wino2 wino4w"), 4, 16, 16, 128, 64, 3, 1, 1, in_act=0.2, bias=True,
        pair=dict(Cin=32, k=3)),
    row("pair_wino_split", ("wino2 wino2 wino4w", "wino2 wino4 wino4w"), 1, 32, 32, 64, 2048, 3, 1, 1, in_act=0.0,
        pair=dict(Cin=64, k=3)),
    row("pair_wino34", ("direct direct direct", "direct wino34 direct"), 2, 16, 19, 64, 64, 4, 1, 1, in_act=0.2, bias=True,
        pair=dict(Cin=32, k=1)),
    row("pair_gemm", ("direct direct direct", "gemm gemm gemm_tn"), 2, 128, 128, 256, 128, 1, 1, 0, in_act=0.0, bias=True,
        pair=dict(Cin=64, k=1)),
    row("pair_direct", ("direct direct direct", "direct direct direct"), 2, 9, 9, 16, 8, 3, 1, 1, in_act=0.2, bias=True,
        pair=dict(Cin=8, k=3)),
    row("pair_direct_s2", ("direct direct direct", "direct direct direct"), 2, 17, 17, 12, 16, 4, 2, 2, in_act=0.0,
        bias=True, pair=dict(Cin=8, k=3)),
    row("pair_linear", ("direct direct direct", "direct direct direct"), 300, 1, 1, 512, 128, 1, 1, 0, in_act=0.0,
        bias=True, pair=dict(Cin=384, k=1), linear=True),
]


def case_ids():
    return [c["name"] for c in CASES]


def plan_args(c):
    """The plan_conv geometry `ops.conv2d` hands `_Conv2d` for row `c` (its channel padding and few-output test), and
    `need` — for the pair rows, of the consumer."""
    from canonicalsg2im_amd import ops
    act, slope = ACTS[c["act"]]
    Cin, Cout = c["Cin"], c["Cout"]
    pc, po = (-Cin) % 4, (-Cout) % 4
    kw = dict(B=c["B"], IH=c["H"], IW=c["W"], KH=c["k"], KW=c["k"], stride=c["s"], pad=c["p"], act=act, slope=slope,
              has_bias=c["bias"], has_res=c["res"], dx_range=c["dx_range"],
              in_act=None if c["in_act"] is None else (LEAKY, c["in_act"]))
    few_raw = (po and Cout + po == 4 and not pc and not c["res"] and not c["packs"] and c["dx_range"] is None
               and c["in_act"] is None and ops.plan_conv(Cin=Cin, Cout=4, cout_real=Cout, **kw).fwd == "few")
    kw.update(Cin=Cin + pc, Cout=Cout if few_raw else Cout + po, cout_real=Cout if Cout + po == 4 else None,
              pre_slope=c["pre_slope"] if (few_raw and Cin < 256) else None,
              packs=True if c["packs"] else None, need=tuple(t in c["need"] for t in "xwb"))
    return kw


def pair_plan_args(c):
    """plan_conv geometry of the producer of a pair row: LeakyReLU(in_act) with bias, stride 1, 'same' padding."""
    k = c["pair"]["k"]
    return dict(B=c["B"], IH=c["H"], IW=c["W"], Cin=c["pair"]["Cin"], Cout=c["Cin"], KH=k, KW=k, stride=1, pad=k // 2,
                act=LEAKY, slope=c["in_act"], has_bias=True, need=(True, True, True))


# ------------------------------------------------------------------------------------ data
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))


def make_data(c):
    """fp32 CPU operands of row `c`: x, w, b, res, dy (and w1, b1 of a pair's producer).  An in_act row's x is its
    producer's output: LeakyReLU(in_act) of Gaussian noise, with exact zeros (a ReLU output has many)."""
    g = _gen(c)
    B, H, W, Cin, Cout, k, s, p = (c[t] for t in ("B", "H", "W", "Cin", "Cout", "k", "s", "p"))
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = {}
    if c["pair"]:
        k1, cin1 = c["pair"]["k"], c["pair"]["Cin"]
        d["x"] = torch.randn(B, cin1, H, W, generator=g)
        d["w1"] = torch.randn(Cin, cin1, k1, k1, generator=g) / (cin1 * k1 * k1) ** 0.5
        d["b1"] = torch.randn(Cin, generator=g) * 0.5
    else:
        x = torch.randn(B, Cin, H, W, generator=g)
        if c["in_act"] is not None:
            x = F.leaky_relu(x, c["in_act"])
            x[:, :, ::3, ::5] = 0.0
        d["x"] = x
    d["w"] = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    d["b"] = torch.randn(Cout, generator=g) if c["bias"] else None
    d["res"] = torch.randn(B, Cout, OH, OW, generator=g) if c["res"] else None
    d["dy"] = torch.randn(B, Cout, OH, OW, generator=g)
    return d


# ------------------------------------------------------------------------------------ the fp64 reference
def _act64(pre, act, slope):
    if act == LEAKY:
        return torch.where(pre > 0, pre, pre * slope), _gate(pre, slope)
    if act == TANH:
        t = torch.tanh(pre)
        return t, 1 - t * t
    return pre, torch.ones_like(pre)


def _gate(x, s):
    """d LeakyReLU(s) / d pre at the output x: 1 where x > 0, else s (the kernels' `x > 0 ? 1 : s`; 0 at ReLU's zeros)."""
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, float(s)))


def kink_mask(pre):
    """1 where the fp64 pre-activation is clear of a LeakyReLU kink by more than fp32 rounding of the sum, else 0."""
    return (pre.abs() > 1e-5 * float(pre.abs().max())).double()


def conv2d_ref64(x, w, b=None, stride=1, pad=0, act=NONE, slope=0.0, res=None, pre_slope=None, in_act=None, dx_range=None,
                 dy=None, need="xwb", gate_x=None):
    """The contract of ops.conv2d in float64 on the CPU, forward and backward written out (no autograd):
    y = act(conv(leaky(x, pre_slope) if pre_slope else x, w) + b) [+ res]; with dy, the gradients of sum(y * dy):
    dx (times where(x > 0, 1, s) for in_act = s — the kernels' gate `x > 0 ? 1 : s`; zero outside channels [lo, hi)
    for dx_range), dw, db, dres = dy.  Only what `need` names ("x", "w", "b", "r") is returned, the rest is None.
    `gate_x`: the tensor whose sign the in_act gate reads, if not x (a pair's producer output at its kinks)."""
    x, w = x.double(), w.double()
    xin = torch.where(x > 0, x, x * pre_slope) if pre_slope is not None else x
    pre = F.conv2d(xin, w, None if b is None else b.double(), stride, pad)
    y, dact = _act64(pre, act, slope)
    if res is not None:
        y = y + res.double()
    out = dict(y=y, pre=pre, dx=None, dw=None, db=None, dres=None)
    if dy is None:
        return out
    gpre = dy.double() * dact
    if "x" in need:
        dx = torch.nn.grad.conv2d_input(x.shape, w, gpre, stride, pad)
        if pre_slope is not None:
            dx = dx * _gate(x, pre_slope)
        if in_act is not None:
            dx = dx * _gate(x if gate_x is None else gate_x.double(), in_act)
        if dx_range is not None:
            keep = torch.zeros(x.shape[1], dtype=torch.float64)
            keep[dx_range[0]:dx_range[1]] = 1.0
            dx = dx * keep.view(1, -1, 1, 1)
        out["dx"] = dx
    if "w" in need:
        out["dw"] = torch.nn.grad.conv2d_weight(xin, w.shape, gpre, stride, pad)
    if "b" in need and b is not None:
        out["db"] = gpre.sum((0, 2, 3))
    if "r" in need and res is not None:
        out["dres"] = dy.double()
    return out


def reference(c, d, gate_x=None):
    """{tensor name: fp64 expectation} of row `c` on data `d` (make_data); None for a gradient not asked for.  The
    incoming gradient is zeroed at the row's own LeakyReLU kinks (written back into d["dy"], the devices use it too)."""
    act, slope = ACTS[c["act"]]
    if c["pair"]:
        k1 = c["pair"]["k"]
        s = c["in_act"]
        p1 = conv2d_ref64(d["x"], d["w1"], d["b1"], 1, k1 // 2, LEAKY, s)
        y1 = p1["y"]
        r2 = conv2d_ref64(y1, d["w"], d["b"], c["s"], c["p"], act, slope, in_act=s, dy=d["dy"], need="xwb",
                          gate_x=gate_x)
        r1 = conv2d_ref64(d["x"], d["w1"], d["b1"], 1, k1 // 2, dy=r2["dx"], need="xwb")
        return dict(y1=y1, y=r2["y"], dx=r1["dx"], dw1=r1["dw"], db1=r1["db"], dw=r2["dw"], db=r2["db"]), p1["pre"]
    if c["act"] in ("relu", "lrelu"):
        pre = conv2d_ref64(d["x"], d["w"], d["b"], c["s"], c["p"], pre_slope=c["pre_slope"])["pre"]
        d["dy"] = (d["dy"].double() * kink_mask(pre)).float()
    r = conv2d_ref64(d["x"], d["w"], d["b"], c["s"], c["p"], act, slope, d["res"], c["pre_slope"], c["in_act"], c["dx_range"],
                     d["dy"], c["need"])
    return {t: r[t] for t in ("y", "dx", "dw", "db", "dres")}, None
