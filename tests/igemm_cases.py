"""The direct-convolution matrix: one row per LAUNCH RULE of csrc/igemm.hip (tests/conv_cases.py has one row per plan).

Three things live here, all host-side and (but for `to_ctypes`) free of the package:

* the launch rules restated in Python from csrc/igemm.hip's host side - `pick_bn`, `pick_split`, `fwd_plan` (uniform
  split-K and the tail split of a partly filled last round), `multi_plan`, `wgrad_plan`, and the workspace bytes that follow
  from them.  tests/test_igemm_cases.py holds them to the library's own workspace queries;
* `desc_ref64` / `wgrad_ref64`: the contract of include/csg_hip.h ("K3/K8/K11") evaluated from the descriptor alone, in
  float64 (or any dtype) on the CPU - the tap table with tap_w, istride, the IHv / IWv bounds with >> in_up, os / ooy / oox
  into an (OHf, OWf) image, x_cs / y_cs slices, bias -> activation -> residual or res_gate -> accumulate onto what y held;
* `CASES`: the rows.  A row is one descriptor (dicts with the C struct's field names), four for the multi entry, with the
  operands it takes and the launch class the restated rules give it, `row["cls"]`.

A forward class is (bn, kind, accumulate, epilogue): kind plain | split (every tile cut along K, k_splitk_epilogue finishes) |
tail (only the m-tiles of the last round are cut); epilogue vec | scalar (Cout or y_cs no multiple of 4).  A weight-gradient
class is (bi, jtiles == 1 | > 1, nsplit == 1 | > 1, db | no db).  `describe(row)` spells out the numbers behind the class.

Buffers (`buffers(row)`): x is (B, IHp, IWp, x_cs) and the kernel reads channels [x_off, x_off + Cin); y (and the residual) is
(B, OHf, OWf, y_cs) and the kernel owns channels [y_off, y_off + Cout) of the grid's pixels - everything else in y is a
sentinel that must survive.  Inputs are seeded from the row's name."""
import zlib

import torch

MAX_TAPS = 16
ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
BM, BK = 128, 32
SENTINEL = -3.25
E_WORKSPACE = "workspace"


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ descriptors
def conv_desc(B, IH, IW, Cin, Cout, KH, KW, stride=1, pad=None, first=0, count=None, x_cs=None, y_cs=None, act=ACT_NONE,
              slope=0.0, accumulate=0, res_gate=0, in_up=0, crop=0):
    """The forward descriptor of taps [first, first + count) of a KH x KW convolution with paddings `pad` = (ph, pw) on a
    (B, IH, IW, Cin) map that the loader upsamples 2^in_up times (nearest) and crops by `crop` rows and columns."""
    ph, pw = (KH // 2, KW // 2) if pad is None else pad
    count = KH * KW - first if count is None else count
    IHv, IWv = (IH << in_up) - crop, (IW << in_up) - crop
    OH, OW = (IHv + 2 * ph - KH) // stride + 1, (IWv + 2 * pw - KW) // stride + 1
    taps = range(first, first + count)
    return dict(B=B, IHp=IH, IWp=IW, Cin=Cin, x_cs=Cin if x_cs is None else x_cs, IHv=IHv, IWv=IWv, in_up=in_up,
                OHg=OH, OWg=OW, OHf=OH, OWf=OW, os=1, ooy=0, oox=0, Cout=Cout, y_cs=Cout if y_cs is None else y_cs,
                istride=stride, ntaps=count, wtaps=KH * KW, tap_dy=[s // KW - ph for s in taps],
                tap_dx=[s % KW - pw for s in taps], tap_w=list(taps), act=act, slope=slope, accumulate=accumulate,
                res_gate=res_gate)


def class_descs(B, IH, IW, Cin, Cout, K, stride, pad, y_cs=None):
    """dX (B, IH, IW, Cin) of a K x K / stride convolution from dY (B, OH, OW, Cout) and weights packed [Cin][K*K][Cout]: one
    descriptor per parity class (py, px) of the input grid.  Input pixel (y, x) receives dY[(y + pad - ky) / stride, ...] *
    w[ky, kx] for the taps whose division is exact - the classes differ in their tap lists and, on odd maps, in their sizes."""
    OH, OW = (IH + 2 * pad - K) // stride + 1, (IW + 2 * pad - K) // stride + 1
    out = []
    for py in range(stride):
        for px in range(stride):
            gh, gw = len(range(py, IH, stride)), len(range(px, IW, stride))
            taps = [(ky, kx) for ky in range(K) for kx in range(K) if (py + pad - ky) % stride == 0 and (px + pad - kx) % stride == 0]
            if gh and gw:
                out.append(dict(B=B, IHp=OH, IWp=OW, Cin=Cout, x_cs=Cout, IHv=OH, IWv=OW, in_up=0, OHg=gh, OWg=gw, OHf=IH, OWf=IW,
                                os=stride, ooy=py, oox=px, Cout=Cin, y_cs=Cin if y_cs is None else y_cs, istride=1,
                                ntaps=len(taps), wtaps=K * K, tap_dy=[(py + pad - ky) // stride for ky, _ in taps],
                                tap_dx=[(px + pad - kx) // stride for _, kx in taps], tap_w=[ky * K + kx for ky, kx in taps],
                                act=ACT_NONE, slope=0.0, accumulate=0, res_gate=0))
    return out


def to_ctypes(d):
    """The package's ctypes mirror of csg_conv_desc, filled from a descriptor dict (the only use of the package in here)."""
    from canonicalsg2im_amd._lib import ConvDesc
    cd = ConvDesc()
    for k, v in d.items():
        if isinstance(v, list):
            for i, t in enumerate(v):
                getattr(cd, k)[i] = t
        else:
            setattr(cd, k, v)
    return cd


def desc_array(descs):
    from canonicalsg2im_amd._lib import ConvDesc
    return (ConvDesc * len(descs))(*[to_ctypes(d) for d in descs])


# ------------------------------------------------------------------------------------------------ the launch rules, restated
def pick_bn(cout):
    return 32 if cout <= 32 else (64 if cout <= 64 else 128)


def pick_split(blocks, steps, min_steps, max_split):
    """The smallest split whose cost (rounds of the 512 resident blocks x steps per split + 0.25 per slab) is within 3 % of
    the best."""
    best, best_cost, s = 1, 1e30, 1
    while s <= max_split and steps // s >= min_steps:
        cost = float(cdiv(blocks * s, 512)) * cdiv(steps, s) + 0.25 * s
        if cost < best_cost * 0.97:
            best, best_cost = s, cost
        s += 1
    return best


def fwd_plan(d):
    M, Ktot, bn = d["B"] * d["OHg"] * d["OWg"], d["ntaps"] * d["Cin"], pick_bn(d["Cout"])
    mtiles, ntiles, nkt = cdiv(M, BM), cdiv(d["Cout"], bn), cdiv(Ktot, BK)
    blocks = mtiles * ntiles
    may_split = nkt >= 16 and d["Cout"] % 4 == 0
    ks = pick_split(blocks, nkt, 8, 64) if blocks < 1024 and may_split else 1
    kt_per = cdiv(nkt, ks)
    p = dict(M=M, Ktot=Ktot, bn=bn, mtiles=mtiles, ntiles=ntiles, nkt=nkt, kt_per=kt_per, ksplit=cdiv(nkt, kt_per), tail=None)
    if 512 < blocks < 4096 and may_split:
        full_mt = (blocks // 512) * 512 // ntiles                   # m-tiles that fit into the whole rounds
        tail_tiles = (mtiles - full_mt) * ntiles
        if full_mt > 0 and 0 < tail_tiles <= 320:
            tks = min(512 // tail_tiles, nkt // 8)
            if tks >= 2:
                p["ksplit"], p["kt_per"] = 1, nkt
                tkp = cdiv(nkt, tks)
                if cdiv(nkt, tkp) >= 2:
                    p["tail"] = dict(tile0=full_mt * ntiles, ks=cdiv(nkt, tkp), kt_per=tkp, m0=full_mt * BM)
    return p


def slab_floats(d, p):
    if p["tail"]:
        return p["tail"]["ks"] * (p["M"] - p["tail"]["m0"]) * d["Cout"]
    return p["ksplit"] * p["M"] * d["Cout"] if p["ksplit"] > 1 else 0


def fwd_workspace_bytes(d):
    return 4 * slab_floats(d, fwd_plan(d))


def multi_plan(descs):
    """One split factor per class, chosen for the grid the classes form TOGETHER; no tail split.  -> (plans with ws_off,
    workspace floats)."""
    plans = []
    for d in descs:
        M, bn = d["B"] * d["OHg"] * d["OWg"], pick_bn(d["Cout"])
        plans.append(dict(M=M, Ktot=d["ntaps"] * d["Cin"], bn=bn, mtiles=cdiv(M, BM), ntiles=cdiv(d["Cout"], bn), tail=None))
    total, off = sum(p["mtiles"] * p["ntiles"] for p in plans), 0
    for d, p in zip(descs, plans):
        nkt = cdiv(p["Ktot"], BK)
        ks = pick_split(total, nkt, 8, 64) if total < 1024 and nkt >= 16 and d["Cout"] % 4 == 0 else 1
        p.update(nkt=nkt, kt_per=cdiv(nkt, ks), ws_off=off)
        p["ksplit"] = cdiv(nkt, p["kt_per"])
        off += slab_floats(d, p)
    return plans, off


def wgrad_plan(d):
    M, Ktot, bi = d["B"] * d["OHg"] * d["OWg"], d["ntaps"] * d["Cin"], pick_bn(d["Cout"])
    itiles, jtiles, nch = cdiv(d["Cout"], bi), cdiv(Ktot, 128), cdiv(M, 32)
    cps = cdiv(nch, pick_split(itiles * jtiles, nch, 8, 256))
    return dict(M=M, Ktot=Ktot, bi=bi, itiles=itiles, jtiles=jtiles, nch=nch, cps=cps, nsplit=cdiv(nch, cps))


def wgrad_workspace_bytes(d):
    p = wgrad_plan(d)                                               # dW slabs + one bias-gradient row per split
    return 4 * p["nsplit"] * d["Cout"] * (d["wtaps"] * d["Cin"] + 1) if p["nsplit"] > 1 else 0


def fwd_class(d, p=None):
    p = fwd_plan(d) if p is None else p
    kind = "tail" if p["tail"] else ("split" if p["ksplit"] > 1 else "plain")
    return (p["bn"], kind, "acc" if d["accumulate"] else "set", "scalar" if (d["Cout"] | d["y_cs"]) & 3 else "vec")


def wgrad_class(d, db):
    p = wgrad_plan(d)
    return (p["bi"], "j1" if p["jtiles"] == 1 else "j>1", "one" if p["nsplit"] == 1 else "split", "db" if db else "nodb")


def chunks_per_split(d):
    """The 32-pixel chunks each pixel split of a weight-gradient launch walks (the last one may be short)."""
    p = wgrad_plan(d)
    return [min(p["nch"], (s + 1) * p["cps"]) - s * p["cps"] for s in range(p["nsplit"])]


def describe(row):
    """(bn, mtiles x ntiles, nkt, ksplit | tail(tile0, ks, m0) | plain, accumulate, vec | scalar) per descriptor;
    (bi, itiles x jtiles, nsplit, cps) for a weight-gradient row."""
    if row["kind"] == "wgrad":
        p = wgrad_plan(row["descs"][0])
        return "bi%d %dx%d nsplit=%d cps=%d%s" % (p["bi"], p["itiles"], p["jtiles"], p["nsplit"], p["cps"], " db" if row["db"] else "")
    plans = multi_plan(row["descs"])[0] if row["entry"] == "multi" else [fwd_plan(d) for d in row["descs"]]
    out = []
    for d, p in zip(row["descs"], plans):
        t = p["tail"]
        how = "tail(%d,%d,%d)" % (t["tile0"], t["ks"], t["m0"]) if t else ("ksplit=%d" % p["ksplit"] if p["ksplit"] > 1 else "plain")
        out.append("bn%d %dx%d nkt=%d %s %s %s" % (p["bn"], p["mtiles"], p["ntiles"], p["nkt"], how, fwd_class(d, p)[2], fwd_class(d, p)[3]))
    return " | ".join(out)


# ------------------------------------------------------------------------------------------------ the contract in float64
def _patch(d, x, t, x_off):
    """(B, OHg, OWg, Cin): what tap slot t reads for every grid point, zeros outside [0, IHv) x [0, IWv)."""
    iy = torch.arange(d["OHg"]) * d["istride"] + d["tap_dy"][t]
    ix = torch.arange(d["OWg"]) * d["istride"] + d["tap_dx"][t]
    vy, vx = (iy >= 0) & (iy < d["IHv"]), (ix >= 0) & (ix < d["IWv"])
    sy, sx = torch.where(vy, iy, 0) >> d["in_up"], torch.where(vx, ix, 0) >> d["in_up"]
    assert int(sy.max()) < d["IHp"] and int(sx.max()) < d["IWp"], "the descriptor reads past the physical map"
    p = x[:, sy][:, :, sx][..., x_off:x_off + d["Cin"]]
    return p * (vy[:, None] & vx[None, :])[None, :, :, None].to(p.dtype)


def desc_ref64(d, x, w, bias=None, res=None, y0=None, x_off=0, y_off=0, dtype=torch.float64):
    """y after csg_conv_fwd(d): a copy of y0 (B, OHf, OWf, y_cs) with channels [y_off, y_off + Cout) of the grid's pixels
    replaced; also the boolean mask of what the launch owns.  x (B, IHp, IWp, x_cs), w (Cout, wtaps, Cin), res like y0."""
    x, w, y = x.to(dtype), w.to(dtype), y0.to(dtype).clone()
    B, OHg, OWg, Cout = d["B"], d["OHg"], d["OWg"], d["Cout"]
    assert tuple(x.shape) == (B, d["IHp"], d["IWp"], d["x_cs"]) and tuple(w.shape) == (Cout, d["wtaps"], d["Cin"])
    assert tuple(y.shape) == (B, d["OHf"], d["OWf"], d["y_cs"])
    acc = torch.zeros(B * OHg * OWg, Cout, dtype=dtype)
    for t in range(d["ntaps"]):
        acc += _patch(d, x, t, x_off).reshape(-1, d["Cin"]) @ w[:, d["tap_w"][t], :].t()
    v = acc.view(B, OHg, OWg, Cout)
    if bias is not None:
        v = v + bias.to(dtype)
    slope = float(torch.tensor(d["slope"], dtype=torch.float32))    # the descriptor's field is a C float
    if d["act"] == ACT_LEAKY:
        v = torch.where(v > 0, v, v * slope)
    elif d["act"] == ACT_TANH:
        v = torch.tanh(v)
    oy = slice(d["ooy"], d["ooy"] + (OHg - 1) * d["os"] + 1, d["os"])
    ox = slice(d["oox"], d["oox"] + (OWg - 1) * d["os"] + 1, d["os"])
    cs = slice(y_off, y_off + Cout)
    if res is not None:
        r = res.to(dtype)[:, oy, ox, cs]
        v = v * torch.where(r > 0, 1.0, slope).to(dtype) if d["res_gate"] else v + r
    if d["accumulate"]:
        v = v + y[:, oy, ox, cs]
    y[:, oy, ox, cs] = v
    own = torch.zeros(y.shape, dtype=torch.bool)
    own[:, oy, ox, cs] = True
    return y, own


def wgrad_ref64(d, x, dy, x_off=0, y_off=0, dtype=torch.float64):
    """dw[n][tap_w][c] = sum_m dy[m][n] * x[src(m, tap)][c] and db[n] = sum_m dy[m][n]; dy (B, OHg, OWg, y_cs)."""
    x, g = x.to(dtype), dy.to(dtype)[..., y_off:y_off + d["Cout"]].reshape(-1, d["Cout"])
    dw = torch.zeros(d["Cout"], d["wtaps"], d["Cin"], dtype=dtype)
    for t in range(d["ntaps"]):
        dw[:, d["tap_w"][t], :] += g.t() @ _patch(d, x, t, x_off).reshape(-1, d["Cin"])
    return dw, g.sum(0)


# ------------------------------------------------------------------------------------------------ rows
CASES = []


def _row(name, kind, descs, **kw):
    row = dict(name=name, kind=kind, descs=descs, bias=False, res=False, x_off=0, y_off=0, db=False, refuse=None,
               short_ws=False, conv=None, cls=None, entry=kind)       # entry: fwd | multi | wgrad, also for a refusal
    row.update(kw)
    if row["refuse"] is None:
        if kind == "wgrad":
            row["cls"] = (wgrad_class(descs[0], row["db"]),)
        elif kind == "multi":
            row["cls"] = tuple(fwd_class(d, p) for d, p in zip(descs, multi_plan(descs)[0]))
        else:
            row["cls"] = tuple(fwd_class(d) for d in descs)
    assert name not in {r["name"] for r in CASES}, name
    CASES.append(row)
    return row


def _fwd(name, B, IH, IW, Cin, Cout, KH, KW, stride=1, pad=None, bias=False, res=False, x_off=0, y_off=0, kind="fwd", **kw):
    ph, pw = (KH // 2, KW // 2) if pad is None else pad
    whole = kw.get("first", 0) == 0 and kw.get("count") is None
    conv = dict(Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=(ph, pw), whole=whole)       # for the F.conv2d cross-check
    extra = dict(refuse=kw.pop("refuse", None), short_ws=kw.pop("short_ws", False), entry="fwd")
    return _row(name, kind, [conv_desc(B, IH, IW, Cin, Cout, KH, KW, stride, (ph, pw), **kw)], bias=bias, res=res, x_off=x_off,
                y_off=y_off, conv=conv, **extra)


# ---- forward tiles and epilogue: block width 32 | 64 | 128 with whole and partial last channel tiles
for _c in (4, 20, 32, 36, 64, 68, 128, 132, 192, 320):
    _fwd("cout%d" % _c, 2, 5, 7, 8, _c, 3, 3, bias=True, act=ACT_LEAKY, slope=0.2)
# rows of the pixel tile: M = 1 | 127 | 128 | 129
for _m, (_h, _w) in ((1, (1, 1)), (127, (1, 127)), (128, (8, 16)), (129, (3, 43))):
    _fwd("m%d" % _m, 1, _h, _w, 8, 8, 3, 3, bias=True)
# a 1x1 map: one 128-row tile spans 128 images (a_base = (b - b0) * img_bytes)
_fwd("map1x1_b300", 300, 1, 1, 8, 8, 3, 3, bias=True)
# the fast division by OW
for _h, _w in ((5, 1), (4, 3), (3, 7), (2, 257)):
    _fwd("ow%d" % _w, 2, _h, _w, 4, 8, 3, 3)
# the scalar epilogue: Cout or y_cs no multiple of 4
for _c, _ycs, _off in ((3, 3, 0), (5, 5, 0), (6, 6, 0), (4, 6, 1)):
    _n = "scalar_c%d_cs%d" % (_c, _ycs)
    _fwd(_n + "_acc", 2, 5, 7, 8, _c, 3, 3, y_cs=_ycs, y_off=_off, accumulate=1)
    _fwd(_n + "_bias_tanh", 2, 5, 7, 8, _c, 3, 3, y_cs=_ycs, y_off=_off, bias=True, act=ACT_TANH)
    _fwd(_n + "_res", 2, 5, 7, 8, _c, 3, 3, y_cs=_ycs, y_off=_off, res=True)
# the vector epilogue, each stage alone and all together
_fwd("vec_none", 2, 5, 7, 8, 8, 3, 3)
_fwd("vec_bias", 2, 5, 7, 8, 8, 3, 3, bias=True)
_fwd("vec_leaky", 2, 5, 7, 8, 8, 3, 3, act=ACT_LEAKY, slope=0.2)
_fwd("vec_tanh", 2, 5, 7, 8, 8, 3, 3, act=ACT_TANH)
_fwd("vec_res", 2, 5, 7, 8, 8, 3, 3, res=True)
_fwd("vec_gate", 2, 5, 7, 8, 8, 3, 3, res=True, res_gate=1, slope=0.2)
_fwd("vec_acc", 2, 5, 7, 8, 8, 3, 3, accumulate=1)
_fwd("vec_bias_tanh_res_acc", 2, 5, 7, 8, 8, 3, 3, bias=True, act=ACT_TANH, res=True, accumulate=1)
_fwd("bn64_acc", 2, 5, 7, 8, 64, 3, 3, accumulate=1)
_fwd("bn128_acc", 2, 5, 7, 8, 128, 3, 3, accumulate=1)
# ---- the K loop: channels per tap (Cin 12 and 20 wrap inside a K tile), every drain case and the steady loop
for _c in (4, 8, 12, 20, 36, 48):
    _fwd("cin%d" % _c, 2, 5, 7, _c, 8, 3, 3)
for _k in range(1, 8):
    _fwd("nkt%d" % _k, 1, 6, 7, 8 * _k, 8, 2, 2, pad=(0, 0))
_fwd("ktot100", 2, 5, 7, 20, 8, 1, 5)                                  # Ktot % 32 != 0, the last tile holds 4 columns
_fwd("taps5x5_first0", 2, 6, 5, 8, 8, 5, 5, first=0, count=16)
_fwd("taps5x5_first16", 2, 6, 5, 8, 8, 5, 5, first=16, count=9)
for _kh, _kw in ((1, 7), (7, 1), (1, 3), (3, 1)):
    for _h, _w in ((5, 5), (7, 5), (1, 1)):
        _fwd("rect%dx%d_on%dx%d" % (_kh, _kw, _h, _w), 2, _h, _w, 8, 12, _kh, _kw, bias=True)
_fwd("stride2_odd", 2, 7, 9, 8, 8, 3, 3, stride=2)
_fwd("stride2_even", 2, 8, 6, 8, 8, 3, 3, stride=2)
_fwd("stride2_4x4", 2, 9, 8, 8, 8, 4, 4, stride=2, pad=(1, 1))
# ---- slices and the folded upsample
_fwd("x_slice", 2, 5, 7, 8, 8, 3, 3, x_cs=16, x_off=4)
_fwd("y_slice", 2, 5, 7, 8, 8, 3, 3, y_cs=20, y_off=4, bias=True)
_fwd("xy_slice_bn128", 2, 5, 7, 8, 68, 3, 3, x_cs=16, x_off=4, y_cs=80, y_off=4)
_fwd("up1_even", 2, 4, 5, 8, 8, 3, 3, in_up=1)
_fwd("up1_odd", 2, 4, 5, 8, 8, 3, 3, in_up=1, crop=1)
_fwd("up1_stride2", 2, 4, 5, 8, 8, 3, 3, stride=2, in_up=1, crop=1)
# ---- uniform split-K: 16 K tiles and up, fewer than 1024 tiles, Cout % 4 == 0
_fwd("nkt15_plain", 2, 3, 3, 480, 8, 1, 1)
_fwd("nkt16_split", 2, 3, 3, 512, 8, 1, 1)
_fwd("nkt17_short_last", 2, 3, 3, 544, 8, 1, 1, bias=True, act=ACT_LEAKY, slope=0.2)
_fwd("ksplit4_m2", 2, 1, 1, 384, 384, 1, 3)
_fwd("cout6_k512_plain", 2, 3, 3, 512, 6, 1, 1)
_fwd("split_acc_5x5", 2, 9, 9, 64, 64, 5, 5, first=16, count=9, accumulate=1)
_fwd("split_res", 2, 3, 3, 512, 8, 1, 1, res=True, bias=True)
_fwd("split_gate", 2, 3, 3, 512, 8, 1, 1, res=True, res_gate=1, slope=0.2)
_fwd("split_y_slice", 2, 3, 3, 512, 8, 1, 1, y_cs=20, y_off=4)
_fwd("split_scalar_cs6", 2, 3, 3, 512, 4, 1, 1, y_cs=6, y_off=1, accumulate=1)     # Cout % 4 == 0 splits, y_cs = 6 is scalar
_fwd("split_bn64", 2, 3, 3, 512, 64, 1, 1, bias=True)
_fwd("split_bn128", 2, 3, 3, 512, 132, 1, 1, bias=True, act=ACT_TANH)
_fwd("refuse_short_workspace", 2, 3, 3, 512, 8, 1, 1, kind="refuse", refuse=E_WORKSPACE, short_ws=True)
# ---- the tail split: a little over a multiple of 512 tiles
_fwd("tail_nt8", 2, 41, 100, 512, 1024, 1, 1, bias=True, act=ACT_LEAKY, slope=0.2)     # M 8200: 2 slabs from row 8192
_fwd("tail_nt4", 4, 41, 100, 512, 512, 1, 1)                                          # M 16400
_fwd("tail_nt1_bn32", 4, 258, 258, 32, 32, 4, 4, stride=2, pad=(1, 1))                # 521 tiles, 2 slabs from row 65536
_fwd("tail_nt2_5slabs", 120, 17, 17, 192, 192, 7, 1, bias=True)                       # Mixed_7a.branch7x7x3_3 at batch 120
_fwd("tail_bn64", 4, 128, 129, 512, 64, 1, 1)                                         # 516 tiles: the last 4 cut in two
_fwd("tail_acc", 2, 41, 100, 512, 1024, 1, 1, accumulate=1)
_fwd("tail_res", 2, 41, 100, 512, 1024, 1, 1, res=True)
_fwd("tail_y_slice", 2, 41, 100, 512, 1024, 1, 1, y_cs=1036, y_off=4)
_fwd("tail_scalar_cs1030_acc", 2, 41, 100, 512, 1024, 1, 1, y_cs=1030, y_off=3, accumulate=1)   # whole tiles: scalar stores
_fwd("m65536_nt1_plain", 4, 128, 128, 512, 32, 1, 1)                                  # exactly 512 tiles: no tail
# ---- refusals of csg_conv_fwd
_fwd("refuse_gate_act", 2, 5, 7, 8, 8, 3, 3, kind="refuse", refuse="res_gate", res=True, res_gate=1, act=ACT_LEAKY, slope=0.2)
_fwd("refuse_gate_acc", 2, 5, 7, 8, 8, 3, 3, kind="refuse", refuse="res_gate", res=True, res_gate=1, accumulate=1)


# ---- multi: the parity classes of a 4x4 / 2 backward-data pass in ONE launch
def _multi(name, B, IH, IW, Cin, Cout, **kw):
    geom = dict(B=B, IH=IH, IW=IW, Cin=Cin, Cout=Cout, K=4, stride=2, pad=1)
    return _row(name, kw.pop("kind", "multi"), kw.pop("descs", None) or class_descs(B, IH, IW, Cin, Cout, 4, 2, 1), conv=geom,
                entry="multi", **kw)


_multi("multi_odd", 2, 9, 7, 8, 32)
_multi("multi_even", 2, 8, 6, 8, 32)
_multi("multi_odd_bias_res", 2, 9, 7, 8, 32, bias=True, res=True)      # the in-kernel epilogue of the multi launch
_multi("multi_odd_split", 2, 9, 7, 8, 128)                             # 4 taps x 128 channels: 16 K tiles, ws_off per class
_multi("multi_even_split_bn64", 1, 6, 6, 36, 160, bias=True, res=True)
_five = class_descs(2, 9, 7, 8, 32, 4, 2, 1)
_multi("refuse_multi_five", 2, 9, 7, 8, 32, kind="refuse", refuse="1..4 descriptors", descs=_five + _five[:1])
_mixed = class_descs(2, 9, 7, 8, 32, 4, 2, 1)
_mixed[2] = dict(_mixed[2], Cout=12, y_cs=12)
_multi("refuse_multi_channels", 2, 9, 7, 8, 32, kind="refuse", refuse="must share channels", descs=_mixed)


# ---- weight gradient: rows = output channels (bi 32 | 64 | 128), columns = (tap, channel) in tiles of 128, pixels in chunks of 32
def _wg(name, B, IH, IW, Cin, Cout, KH, KW, stride=1, pad=None, db=False, x_off=0, y_off=0, kind="wgrad", refuse=None, **kw):
    ph, pw = (KH // 2, KW // 2) if pad is None else pad
    conv = dict(Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=(ph, pw), whole=True)
    return _row(name, kind, [conv_desc(B, IH, IW, Cin, Cout, KH, KW, stride, (ph, pw), **kw)], db=db, x_off=x_off, y_off=y_off,
                conv=conv, refuse=refuse, entry="wgrad")


for _c in (32, 36, 64, 68, 128, 160):
    _wg("wg_cout%d" % _c, 2, 5, 7, 8, _c, 3, 3, db=_c in (32, 64, 128))
_wg("wg_ktot128", 2, 5, 7, 128, 32, 1, 1, db=True)
_wg("wg_ktot132", 2, 5, 7, 132, 32, 1, 1)
for _m, (_h, _w) in ((31, (1, 31)), (32, (4, 8)), (33, (3, 11)), (255, (15, 17)), (257, (1, 257))):
    _wg("wg_m%d" % _m, 1, _h, _w, 8, 32, 3, 3, db=_m in (31, 33, 257))
for _k, (_h, _w) in ((3, (9, 10)), (4, (9, 14)), (5, (10, 15)), (6, (11, 17)), (7, (7, 31))):       # 3 .. 7 chunks, one split
    _wg("wg_chunks%d" % _k, 1, _h, _w, 8, 32, 3, 3, db=_k % 2 == 1)
_wg("wg_split12_db", 2, 40, 40, 64, 160, 3, 3, db=True)
_wg("wg_split12", 2, 40, 40, 64, 160, 3, 3)
_wg("wg_split3", 3, 33, 33, 36, 32, 4, 4, stride=2, pad=(1, 1))
_wg("wg_split3_db", 3, 33, 33, 36, 32, 4, 4, stride=2, pad=(1, 1), db=True)
_wg("wg_66564_terms", 4, 258, 258, 32, 32, 4, 4, stride=2, pad=(1, 1), db=True)
_wg("wg_y_slice", 2, 5, 7, 8, 32, 3, 3, db=True, y_cs=44, y_off=4)
_wg("wg_x_slice", 2, 5, 7, 8, 32, 3, 3, x_cs=16, x_off=4)
_wg("wg_up1_even", 2, 4, 5, 8, 32, 3, 3, db=True, in_up=1)
_wg("wg_up1_odd", 2, 4, 5, 8, 32, 3, 3, in_up=1, crop=1)
_wg("refuse_wg_partial_taps", 2, 6, 5, 8, 32, 5, 5, kind="refuse", refuse="every weight tap must be listed", first=0, count=16)

# ---- the Python entry: ops.conv2d_forward(x, w [Cout][KH][KW][Cin], bias, ReLU) into channels [off, off + Cout) of `wide`
ENTRY_CASES = (
    dict(name="entry_5x5_split_acc", B=2, H=9, W=9, Cin=64, Cout=64, KH=5, KW=5, pad=(2, 2), wide=76, off=4),
    dict(name="entry_1x7_tail", B=120, H=17, W=17, Cin=192, Cout=192, KH=1, KW=7, pad=(0, 3), wide=208, off=8),
)


def entry_descs(e):
    """The launches conv2d_forward makes for an entry row: ceil(taps / 16) descriptors over the one weight, the first writes,
    the others accumulate; with more than one, bias and activation wait for csg_bias_act."""
    taps = e["KH"] * e["KW"]
    single = taps <= MAX_TAPS
    return [conv_desc(e["B"], e["H"], e["W"], e["Cin"], e["Cout"], e["KH"], e["KW"], 1, e["pad"], first=f,
                      count=min(MAX_TAPS, taps - f), y_cs=e["wide"], act=ACT_LEAKY if single else ACT_NONE, accumulate=1 if f else 0)
            for f in range(0, taps, MAX_TAPS)]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


# ------------------------------------------------------------------------------------------------ operands
def buffers(row):
    """{name: shape} of what the device test allocates for the row (float32); every address the descriptors can produce must
    lie inside (tests/test_igemm_cases.py checks that on the CPU, before any row reaches a device)."""
    d = row["descs"][0]
    out = dict(x=(d["B"], d["IHp"], d["IWp"], d["x_cs"]), w=(d["Cout"], d["wtaps"], d["Cin"]))
    if row["entry"] == "wgrad":
        out.update(dy=(d["B"], d["OHg"], d["OWg"], d["y_cs"]), dw=(d["Cout"], d["wtaps"], d["Cin"]), db=(d["Cout"],))
    else:
        out.update(y=(d["B"], d["OHf"], d["OWf"], d["y_cs"]), bias=(d["Cout"],))
    return out


def make_data(row):
    """Seeded float32 operands: x, w (He-scaled over the listed taps), and per kind bias, res (for res_gate a third exact
    zeros, the rest of both signs), y0 (seeded where the row accumulates, the sentinel elsewhere) or dy."""
    g = torch.Generator().manual_seed(zlib.crc32(row["name"].encode()))
    d, shapes = row["descs"][0], buffers(row)
    ntaps = max(dd["ntaps"] for dd in row["descs"])
    out = dict(x=torch.randn(shapes["x"], generator=g), w=torch.randn(shapes["w"], generator=g) * (1.0 / (ntaps * d["Cin"])) ** 0.5)
    if "dy" in shapes:
        out["dy"] = torch.randn(shapes["dy"], generator=g)
        return out
    out["bias"] = 0.3 * torch.randn(shapes["bias"], generator=g) if row["bias"] else None
    out["res"] = None
    if row["res"]:
        r = torch.randn(shapes["y"], generator=g)
        out["res"] = torch.where(torch.rand(shapes["y"], generator=g) < 1 / 3, torch.zeros(()), r) if d["res_gate"] else r
    acc = any(dd["accumulate"] for dd in row["descs"])
    out["y0"] = torch.randn(shapes["y"], generator=g) if acc else torch.full(shapes["y"], SENTINEL)
    return out


def reference(row, data, dtype=torch.float64):
    """{tensor: value in `dtype`} plus "own" (forward kinds): the descriptors applied in order to y0."""
    if row["kind"] == "wgrad":
        dw, db = wgrad_ref64(row["descs"][0], data["x"], data["dy"], row["x_off"], row["y_off"], dtype)
        return dict(dw=dw, db=db if row["db"] else None)
    y, own = data["y0"], torch.zeros(data["y0"].shape, dtype=torch.bool)
    for d in row["descs"]:
        y, o = desc_ref64(d, data["x"], data["w"], data["bias"], data["res"], y, row["x_off"], row["y_off"], dtype)
        own |= o
    return dict(y=y, own=own)


# ------------------------------------------------------------------------------------------------ the Inception census
# The layers of Inception-v3 that reach ops.conv2d_forward (canonicalsg2im_amd/inception.py): every rectangular or 5x5 layer,
# and every layer that ends a branch and writes into the block's output.  (block kind: names of the branch ends)
BRANCH_ENDS = {"A": ("branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"), "B": ("branch3x3", "branch3x3dbl_3"),
               "C": ("branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool"), "D": ("branch3x3_2", "branch7x7x3_4"),
               "E": ("branch1x1", "branch3x3_2a", "branch3x3_2b", "branch3x3dbl_3a", "branch3x3dbl_3b", "branch_pool")}
BLOCK_MAP = {"A": 35, "B": 35, "C": 17, "D": 17, "E": 8}              # the map a block's layers read (stride-2 ends halve it)


def census(layers, blocks, batches=(1, 2, 50)):
    """{(layer name, batch): [class of each launch]} for `layers` = [(name, cin, cout, kh, kw, stride, ph, pw)] of the Mixed
    blocks `blocks` = [(block name, kind)]."""
    out = {}
    kinds = dict(blocks)
    for name, cin, cout, kh, kw, stride, ph, pw in layers:
        blk, _, leaf = name.partition(".")
        if blk not in kinds or not (leaf in BRANCH_ENDS[kinds[blk]] or kh != kw or kh * kw > MAX_TAPS):
            continue
        side = BLOCK_MAP[kinds[blk]]
        for B in batches:
            taps = kh * kw
            out[(name, B)] = [fwd_class(conv_desc(B, side, side, cin, cout, kh, kw, stride, (ph, pw), first=f,
                                                  count=min(MAX_TAPS, taps - f), accumulate=1 if f else 0))
                              for f in range(0, taps, MAX_TAPS)]
    return out
