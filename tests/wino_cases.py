"""The Winograd matrix: one row per LAUNCH RULE of csrc/wino.hip, csrc/wino4.hip and csrc/wino4w.hip, whose host side is
csrc/csg_wino_host.h (tests/conv_cases.py has one row per plan of `ops.conv2d`; tests/igemm_cases.py is the direct
convolution's matrix).

Three things live here, all host-side and (but for `to_ctypes`) free of the package:

* the launch rules restated in Python from the code - `wn_plan`, `w4_plan`, `w4_persistent_blocks`, `wn_wg_plan`, `ww_plan`,
  `wino_split_plan`, `wino_wg_slice_plan`, `wino_wg_workspace`, `wino_pack_bytes` - and the workspace bytes that follow from
  them.  tests/test_wino_cases.py holds them to the library's own queries;
* `wino_ref64` / `wino_wgrad_ref64`: the contract of include/csg_hip.h ("K8w", "K8w4", "K8w34") evaluated from the descriptor
  alone, in float64 (or any dtype) on the CPU, tap by tap - x read at channels [x_off, x_off + Cin) of (B, H, W, x_cs), y
  written at [y_off, y_off + Cout) of (B, Ho, Wo, y_cs), bias -> activation -> + residual -> * (gate > 0 ? 1 : gate_slope),
  the backward-data operand, sigma, the SPADE modulation of csg_wino4_conv_part / csg_wino4_conv_spade;
* `CASES`: the rows.  A row is one descriptor (a dict with the C struct's field names) with the operands it takes and the
  launch class the restated rules give it, `row["cls"]`: a set of (family, axis, value) triples.  `all_classes()` is the
  full set the rules enumerate; tests/test_wino_cases.py asserts that the rows reach exactly that set.

Families: f2 = F(2x2,3x3) csg_wino_conv, f4 = F(4x4,3x3) csg_wino4_conv / _conv_part / _conv_spade, f34 = F(3x3,4x4)
csg_wino34_conv, wg2 = F(3x3,2x2) csg_wino_bwd_weight, wg4 = F(3x3,4x4) csg_wino4_bwd_weight.

Buffers (`buffers(row)`): every channel of x, dy, residual, gate, mod_x and mod_gamma outside the slice the kernel may
read holds NaN; every entry of y and gamma_out holds the sentinel -3.25, and the launch owns channels [y_off, y_off + Cout)
of every pixel - everything else must survive.  Slice offsets are multiples of 4 floats (16-byte alignment).  Inputs are
seeded from the row's name.

The convolution entries take a dense x only: `wn_plan` / `w4_plan` refuse x_cs != Cin (csg_wino_host.h says why), the
refusal rows `refuse_*_strided_x` hold every entry to that, and the class axis "strided-y" names what their rows vary.  The
weight gradients take x with its channel stride: their rows reach "strided-x" and "strided-y"."""
import zlib

import torch

ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
E_BADSHAPE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
SENTINEL = -3.25
MAX_RECORDS = 0x7FFFFFF0
CUS = 256                     # compute units of the part the table's persistent rows are sized for (MI355X)
OFF = 4                       # where a strided row's slice begins, in floats


def cdiv(a, b):
    return (a + b - 1) // b


def wino_desc(B, H, W, Cin, Cout, x_cs=None, y_cs=None, act=ACT_NONE, slope=0.0):
    return dict(B=B, H=H, W=W, Cin=Cin, x_cs=Cin if x_cs is None else x_cs, Cout=Cout, y_cs=Cout if y_cs is None else y_cs,
                act=act, slope=slope)


def to_ctypes(d):
    """The package's ctypes mirror of csg_wino_desc, filled from a descriptor dict (the only use of the package in here)."""
    from canonicalsg2im_amd._lib import WinoDesc
    cd = WinoDesc()
    for k, v in d.items():
        setattr(cd, k, v)
    return cd


# ------------------------------------------------------------------------------------------------ the launch rules, restated
def wino_desc_check(d, positions, pixels):
    """0, or the code csg_wino_host.h's wino_desc_check refuses the descriptor with."""
    if min(d["B"], d["H"], d["W"], d["Cin"], d["Cout"]) <= 0:
        return E_BADSHAPE
    if d["Cin"] % 4 or d["x_cs"] % 4 or d["x_cs"] < d["Cin"] or d["Cout"] % 4 or d["y_cs"] % 4 or d["y_cs"] < d["Cout"]:
        return E_UNSUPPORTED
    if pixels * max(d["x_cs"], d["y_cs"]) * 4 >= MAX_RECORDS:
        return E_UNSUPPORTED
    if positions * cdiv(d["Cout"], 32) * cdiv(d["Cin"], 8) * 1024 >= MAX_RECORDS:
        return E_UNSUPPORTED
    return 0


def wn_plan(d):
    """F(2x2,3x3): a block owns TW x TH = 32 tiles of 2x2 pixels and 32 * ntb output channels; stages of 16 channels."""
    rc = wino_desc_check(d, 16, d["B"] * d["H"] * d["W"])
    if rc:
        return rc
    if d["x_cs"] != d["Cin"]:                                       # wino_conv_dense_x: the convolution entries take a dense x
        return E_UNSUPPORTED
    if d["H"] % 2 or d["W"] % 2 or d["W"] < 8 or d["Cin"] % 16:
        return E_UNSUPPORTED
    TW = 16 if d["W"] >= 32 else (8 if d["W"] >= 16 else 4)
    TH = 32 // TW
    ntb = 1 if d["Cout"] <= 32 else 2
    return dict(TW=TW, TH=TH, tbx=cdiv(d["W"] // 2, TW), tby=cdiv(d["H"] // 2, TH), ntb=ntb, nblocks=cdiv(d["Cout"], 32 * ntb),
                NT32=cdiv(d["Cout"], 32), Q8=cdiv(d["Cin"], 8), nstage=cdiv(d["Cin"], 16), ksplit=1, sps=cdiv(d["Cin"], 16),
                Ho=d["H"], Wo=d["W"], slab=d["B"] * d["H"] * d["W"] * d["y_cs"], B=d["B"], Cout=d["Cout"], y_cs=d["y_cs"],
                gb_off=0)


def w4_plan(d, T, pad=1):
    """T = 4: F(4x4,3x3), pad 1.  T = 3: F(3x3,4x4), pad 1 | 2, output = input + 2 pad - 3.  A block owns 8 x 4 tiles of
    T x T pixels and 64 output channels; stages of 8 channels."""
    rc = wino_desc_check(d, 36, d["B"] * (d["H"] + 1) * (d["W"] + 1))
    if rc:
        return rc
    if d["x_cs"] != d["Cin"]:
        return E_UNSUPPORTED
    if T == 4:
        if d["H"] % 4 or d["W"] % 4 or d["W"] < 32 or d["H"] < 16:
            return E_UNSUPPORTED
    elif pad not in (1, 2) or d["H"] + 2 * pad < 4 or d["W"] + 2 * pad < 4:
        return E_UNSUPPORTED
    Ho, Wo = (d["H"], d["W"]) if T == 4 else (d["H"] + 2 * pad - 3, d["W"] + 2 * pad - 3)
    if d["Cin"] % 8:
        return E_UNSUPPORTED
    return dict(T=T, pad=pad, Ho=Ho, Wo=Wo, tbx=cdiv(Wo, T * 8), tby=cdiv(Ho, T * 4), nblocks=cdiv(d["Cout"], 64),
                NT32=cdiv(d["Cout"], 32), Q8=cdiv(d["Cin"], 8), nstage=d["Cin"] // 8, ksplit=1, sps=d["Cin"] // 8,
                slab=d["B"] * Ho * Wo * d["y_cs"], B=d["B"], Cout=d["Cout"], y_cs=d["y_cs"], gb_off=0)


SPLIT_RULE = {"f2": (16, 8), "f4": (32, 16), "f34": (32, 16)}      # (stages a split needs, stages it leaves to a range)


def wino_split_plan(p, plain, min_stages, min_range):
    """Cut the stages of a launch of fewer than 384 blocks towards 512 blocks: only without an epilogue and with a dense y.
    -> the first ks the rule tried (None: no split), p gets ksplit and sps."""
    if not plain or p["y_cs"] != p["Cout"]:
        return None
    blocks = p["B"] * p["tby"] * p["tbx"] * p["nblocks"]
    if blocks >= 384 or p["nstage"] < min_stages:
        return None
    ks = min(cdiv(512, blocks), p["nstage"] // min_range)
    if ks < 2:
        return None
    p["sps"] = cdiv(p["nstage"], ks)
    p["ksplit"] = cdiv(p["nstage"], p["sps"])
    return ks


def conv_plan(fam, d, pad=1, plain=None):
    """The plan of a convolution entry (an int: the code it is refused with).  `plain`: no epilogue at all, as
    wino_conv_entry sees the call; None: as the workspace query sees the descriptor (no activation)."""
    p = wn_plan(d) if fam == "f2" else w4_plan(d, 4 if fam == "f4" else 3, pad)
    if isinstance(p, int):
        return p
    p["first_ks"] = wino_split_plan(p, d["act"] == ACT_NONE if plain is None else plain, *SPLIT_RULE[fam])
    return p


def conv_workspace_bytes(fam, d, pad=1):
    p = conv_plan(fam, d, pad)
    if isinstance(p, int):
        return -1
    return p["ksplit"] * p["slab"] * 4 if p["ksplit"] > 1 else 0


def w4_persistent_blocks(p, items, cus=CUS):
    """Blocks of the persistent form of k_wino4_conv_v: one per CU, a multiple of 8; 0: the launch runs one block per item."""
    g = cus & ~7 if cus >= 8 else 0
    if g == 0 or p["ksplit"] != 1 or p["nstage"] & 1 or p["nstage"] < 4 or (p["gb_off"] == 0 and p["Cout"] & 63) or items < 2 * g:
        return 0
    return g


def w4_spade_plan(d, cus=CUS):
    """csg_wino4_conv_spade: a block owns the gamma tile and the beta tile of 32 channels; the persistent form only."""
    if d["Cout"] % 32:
        return E_UNSUPPORTED
    p = w4_plan(d, 4)
    if isinstance(p, int):
        return p
    tiles = d["Cout"] // 32
    p.update(NT32=2 * tiles, nblocks=tiles, gb_off=tiles)
    if not w4_persistent_blocks(p, p["B"] * p["tby"] * p["tbx"] * p["nblocks"], cus):
        return E_UNSUPPORTED
    return p


def wino4_supported(d):
    return int(d["H"] % 4 == 0 and d["W"] % 4 == 0 and d["W"] >= 32 and d["H"] >= 16 and d["Cin"] % 8 == 0 and d["Cout"] % 4 == 0)


def wino34_supported(d, pad):
    """What the planner asks before it takes F(3x3,4x4): narrower than what w4_plan serves (maps from 15 pixels, 64 -> 32
    channels up: below that the tile grid is mostly padding)."""
    return int(pad in (1, 2) and d["H"] >= 15 and d["W"] >= 15 and d["Cin"] % 8 == 0 and d["Cout"] % 4 == 0 and d["Cin"] >= 64
               and d["Cout"] >= 32)


def wino_wg_slice_plan(p, tiles2d, target_blocks, min_regions, max_slices):
    nr = p["B"] * p["RXn"] * p["RYn"]
    ns = max(1, min(cdiv(target_blocks, tiles2d), cdiv(nr, min_regions), max_slices))
    p["nregions"], p["rps"] = nr, cdiv(nr, ns)
    p["nsplit"] = cdiv(nr, p["rps"])
    return p


def wn_wg_plan(d):
    """F(3x3,2x2): regions of TSX x 16/TSX tiles; a block owns 64 output x 32 input channels of a slice of the regions."""
    rc = wino_desc_check(d, 0, d["B"] * d["H"] * d["W"] + d["W"] + 1)
    if rc:
        return rc
    tsx = 16 if d["W"] >= 32 else (8 if d["W"] >= 16 else 4)
    tsy = 16 // tsx
    if d["W"] < 8 or d["W"] % (2 * tsx) or d["H"] % (2 * tsy):
        return E_UNSUPPORTED
    p = dict(B=d["B"], tsx=tsx, tsy=tsy, RXn=d["W"] // (2 * tsx), RYn=d["H"] // (2 * tsy), cblocks=cdiv(d["Cout"], 64),
             kblocks=cdiv(d["Cin"], 32))
    p = wino_wg_slice_plan(p, p["cblocks"] * p["kblocks"], 1024, 8, 512)
    p["nslab"] = p["nsplit"]
    return p


def ww_plan(d):
    """F(3x3,4x4): regions of 8 x 8 pixels; a block owns 64 x 64 channels and half of the positions: two slabs per slice."""
    rc = wino_desc_check(d, 0, d["B"] * d["H"] * d["W"] + d["W"] + 1)
    if rc:
        return rc
    if d["W"] % 8 or d["H"] % 8:
        return E_UNSUPPORTED
    p = dict(B=d["B"], RXn=d["W"] // 8, RYn=d["H"] // 8, cblocks=cdiv(d["Cout"], 64), kblocks=cdiv(d["Cin"], 64))
    p = wino_wg_slice_plan(p, p["cblocks"] * p["kblocks"] * 2, 256, 16, 256)
    p["nslab"] = 2 * p["nsplit"]
    return p


def wg_plan(fam, d):
    return wn_wg_plan(d) if fam == "wg2" else ww_plan(d)


def wino_wg_workspace(d, nslab):
    return nslab * d["Cout"] * (9 * d["Cin"] + 1) * 4


def wg_workspace_bytes(fam, d):
    p = wg_plan(fam, d)
    return -1 if isinstance(p, int) else wino_wg_workspace(d, p["nslab"])


def wino_pack_bytes(positions, N, K):
    return -1 if N <= 0 or K <= 0 else positions * cdiv(N, 32) * cdiv(K, 8) * 64 * 16


POSITIONS = {"f2": 16, "f4": 36, "f34": 36}


def pack_geometry(row):
    """(O, I, taps side, N, K): the weight (O, I, k, k) of the row and the extents of its packed operand."""
    d, k = row["d"], 4 if row["fam"] == "f34" else 3
    if row["bwd"]:
        O, I = d["Cin"], d["Cout"]                                    # dX = conv(dY, flipped W^T): N = I, K = O
        return O, I, k, I, O
    O = d["Cout"]
    if row["entry"] == "part":
        O = 32 * row["part"]["tiles_total"]
    elif row["entry"] == "spade":
        O = 2 * d["Cout"]
    return O, d["Cin"], k, O, d["Cin"]


# ------------------------------------------------------------------------------------------------ classes
EPILOGUES = ("none", "bias", "leaky", "tanh", "res", "gate", "bias+leaky+res+gate")
KINDS = ("plain", "split", "unsplit-short-workspace", "unsplit-strided-y")


def epilogue_of(row):
    parts = [n for n, on in (("bias", row["bias"]), ("leaky", row["d"]["act"] == ACT_LEAKY), ("tanh", row["d"]["act"] == ACT_TANH),
                             ("res", row["res"]), ("gate", row["gate"])) if on]
    return "+".join(parts) or "none"


def run_plan(row, cus=CUS):
    """The plan of the launch the row makes (what wino_conv_entry does with the workspace it is given included), and its
    kind: plain | split | unsplit-short-workspace | unsplit-strided-y (a dense twin of the descriptor would split)."""
    fam, d = row["fam"], row["d"]
    plain = epilogue_of(row) == "none"
    p = conv_plan(fam, d, row["pad"], plain)
    kind = "plain"
    if p["ksplit"] > 1:
        kind = "split"
        if row["ws"] != "given":
            kind = "unsplit-short-workspace"
            p["ksplit"], p["sps"] = 1, p["nstage"]
    elif plain and d["y_cs"] != d["Cout"] and conv_plan(fam, dict(d, y_cs=d["Cout"]), row["pad"], True)["ksplit"] > 1:
        kind = "unsplit-strided-y"
    return p, kind


def stage_class(n):
    return "1" if n == 1 else ("2" if n == 2 else ("odd" if n & 1 else "even>=4"))


def classify(row, cus=CUS):
    """The set of (family, axis, value) triples a row reaches."""
    fam, d, out = row["fam"], row["d"], set()
    sx, strided = d["x_cs"] != d["Cin"], d["y_cs"] != d["Cout"]     # convolution rows: x is dense, `strided` is y's
    if row["entry"] == "wgrad":
        p = wg_plan(fam, d)
        db = "db" if row["db"] else "nodb"
        if fam == "wg2":
            out |= {(fam, "launch", (p["tsx"], "direct" if p["nsplit"] == 1 else "summed", db))}
            out |= {(fam, ax, p["tsx"]) for ax, on in (("strided-x", sx), ("strided-y", strided)) if on}
        else:
            out |= {(fam, "launch", ("one-slice" if p["nsplit"] == 1 else "sliced", db))}
            out |= {(fam, ax, True) for ax, on in (("strided-x", sx), ("strided-y", strided)) if on}
        if d["Cin"] % 32 or d["Cout"] % 64:
            out.add((fam, "tail", ("cin" if d["Cin"] % 32 else "") + ("cout" if d["Cout"] % 64 else "")))
        return out
    if row["entry"] == "spade":
        p = w4_spade_plan(d, cus)
        out |= {(fam, "entry", "spade+gamma_out" if row["spade"]["gamma_out"] else "spade"), (fam, "form", "persistent"),
                (fam, "nstage", stage_class(p["nstage"]))}
        if strided:
            out.add((fam, "strided-y", "persistent"))
    else:
        p, kind = run_plan(row, cus)
        out |= {(fam, "kind", kind), (fam, "epilogue", epilogue_of(row))}
        if kind == "split":
            out.add((fam, "split", "uneven" if p["nstage"] % p["sps"] else "even"))
            if p["ksplit"] < p["first_ks"]:
                out.add((fam, "split", "ksplit<ks"))
        if fam == "f2":
            out.add((fam, "tile", (p["TW"], p["ntb"])))
            if strided:
                out.add((fam, "strided-y", p["TW"]))
        elif fam == "f4":
            form = "persistent" if w4_persistent_blocks(p, p["B"] * p["tby"] * p["tbx"] * p["nblocks"] * p["ksplit"], cus) else "one-item"
            entry = "whole" if row["entry"] == "conv" else ("part+mod" if row["part"]["mod"] else "part")
            out |= {(fam, "form", form), (fam, "nstage", stage_class(p["nstage"])), (fam, "entry", entry)}
            if strided:
                out.add((fam, "strided-y", form))
        else:
            out.add((fam, "pad", row["pad"]))
            if strided:
                out.add((fam, "strided-y", True))
    # the pack the row's operand went through
    O, I, k, N, K = pack_geometry(row)
    out |= {(fam, "pack", row["wfmt"]), (fam, "pack", "bwd" if row["bwd"] else "fwd")}
    if row["sigma"]:
        out.add((fam, "pack", "sigma"))
    if N % 32:
        out.add((fam, "pack", "n-tail"))
    return out


def all_classes():
    """Every (family, axis, value) the restated rules can produce and the issue asks a row for."""
    out = set()
    for fam in ("f2", "f4", "f34"):
        kinds = KINDS if fam != "f34" else ("plain", "split")
        out |= {(fam, "kind", k) for k in kinds} | {(fam, "epilogue", e) for e in EPILOGUES} | {(fam, "split", "even")}
        out |= {(fam, "pack", v) for v in ("contig", "fwd", "bwd", "sigma", "n-tail")}
    out |= {("f2", "pack", "cl"), ("f2", "pack", "slice"), ("f4", "pack", "cl"), ("f4", "pack", "slice"), ("f34", "pack", "slice")}
    out |= {("f2", "tile", (tw, ntb)) for tw in (4, 8, 16) for ntb in (1, 2)} | {("f2", "strided-y", tw) for tw in (4, 8, 16)}
    out |= {("f2", "split", "uneven"), ("f2", "split", "ksplit<ks"), ("f4", "split", "uneven")}
    out |= {("f4", "form", f) for f in ("one-item", "persistent")} | {("f4", "strided-y", f) for f in ("one-item", "persistent")}
    out |= {("f4", "nstage", s) for s in ("1", "2", "odd", "even>=4")}
    out |= {("f4", "entry", e) for e in ("whole", "part", "part+mod", "spade", "spade+gamma_out")}
    out |= {("f34", "pad", 1), ("f34", "pad", 2), ("f34", "strided-y", True)}
    out |= {("wg2", "launch", (t, s, b)) for t in (4, 8, 16) for s in ("direct", "summed") for b in ("db", "nodb")}
    out |= {("wg2", ax, t) for t in (4, 8, 16) for ax in ("strided-x", "strided-y")} | {("wg2", "tail", t) for t in ("cin", "cout", "cincout")}
    out |= {("wg4", "launch", (s, b)) for s in ("one-slice", "sliced") for b in ("db", "nodb")}
    out |= {("wg4", "strided-x", True), ("wg4", "strided-y", True), ("wg4", "tail", "cincout")}
    return out


def describe(row):
    """The numbers behind the class, for the report."""
    fam, d = row["fam"], row["d"]
    if row["entry"] == "wgrad":
        p = wg_plan(fam, d)
        return "%s %dx%d regions %d nsplit=%d rps=%d%s" % (fam, p["cblocks"], p["kblocks"], p["nregions"], p["nsplit"], p["rps"],
                                                          " db" if row["db"] else "")
    if row["entry"] == "spade":
        p = w4_spade_plan(d)
        return "f4 spade persistent items=%d nstage=%d%s" % (p["B"] * p["tby"] * p["tbx"] * p["nblocks"], p["nstage"],
                                                             " gamma_out" if row["spade"]["gamma_out"] else "")
    p, kind = run_plan(row)
    items = p["B"] * p["tby"] * p["tbx"] * p["nblocks"]
    how = "split ksplit=%d sps=%d" % (p["ksplit"], p["sps"]) if kind == "split" else kind
    if fam == "f2":
        head = "f2 TW%d NTB%d" % (p["TW"], p["ntb"])
    elif fam == "f4":
        head = "f4 %s %s" % ("persistent" if w4_persistent_blocks(p, items * p["ksplit"]) else "one-item", row["entry"])
    else:
        head = "f34 pad%d" % row["pad"]
    return "%s blocks=%d nstage=%d %s %s" % (head, items, p["nstage"], how, epilogue_of(row))


# ------------------------------------------------------------------------------------------------ the contract in float64
def _taps(xs, w, pad, dtype):
    """sum over taps (a, b) of x[.., y + a - pad, x + b - pad, :] @ w[:, :, a, b]^T: (B, Ho, Wo, O) from NHWC xs and w (O, I, k, k)."""
    B, H, W, _ = xs.shape
    k = w.shape[2]
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, xs.shape[3], dtype=dtype)
    xp[:, pad:pad + H, pad:pad + W] = xs
    acc = torch.zeros(B * Ho * Wo, w.shape[0], dtype=dtype)
    for a in range(k):
        for b in range(k):
            acc += xp[:, a:a + Ho, b:b + Wo].reshape(B * Ho * Wo, -1) @ w[:, :, a, b].t()
    return acc.view(B, Ho, Wo, -1)


def effective_weight(row, data, dtype):
    """(N, K, k, k): the weight the launch convolves with - W / sigma, and for the backward-data operand flipped and
    channel-transposed."""
    w = data["w"].to(dtype)
    if data["sigma"] is not None:
        w = w / data["sigma"].to(dtype)
    return w.flip(2, 3).transpose(0, 1) if row["bwd"] else w


def _leaky(v, slope, dtype):
    return torch.where(v > 0, v, v * torch.tensor(float(torch.tensor(slope, dtype=torch.float32)), dtype=dtype))


def wino_ref64(row, data, dtype=torch.float64):
    """{y, own[, gamma_out]}: y after the row's launch - a copy of y0 (B, Ho, Wo, y_cs) with channels [y_off, y_off + Cout)
    replaced - and the mask of what the launch owns."""
    d, fam = row["d"], row["fam"]
    Cin, Cout, xo, yo = d["Cin"], d["Cout"], row["x_off"], row["y_off"]
    xs = data["x"].to(dtype)[..., xo:xo + Cin]
    assert tuple(data["x"].shape) == (d["B"], d["H"], d["W"], d["x_cs"]) and bool(torch.isfinite(xs).all())
    w = effective_weight(row, data, dtype)
    v = _taps(xs, w, row["pad"], dtype)
    if data["bias"] is not None:
        v = v + data["bias"].to(dtype)
    own_c = slice(yo, yo + Cout)
    out = {}
    if row["entry"] == "part":
        t0 = 32 * row["part"]["tile_off"]
        v = v[..., t0:t0 + Cout]                                       # the slice of the outputs; bias points at its first channel
        if row["part"]["mod"]:
            go = row["part"]["g_off"]
            xh = (data["mod_x"].to(dtype)[..., own_c] - data["mean"].to(dtype)) * data["invstd"].to(dtype)
            v = _leaky(xh * (1 + data["mod_gamma"].to(dtype)[..., go:go + Cout]) + v, row["part"]["mod_slope"], dtype)
    elif row["entry"] == "spade":
        gamma, beta = v[..., :Cout], v[..., Cout:]
        xh = (data["mod_x"].to(dtype)[..., own_c] - data["mean"].to(dtype)) * data["invstd"].to(dtype)
        v = _leaky(xh * (1 + gamma) + beta, row["spade"]["mod_slope"], dtype)
        if row["spade"]["gamma_out"]:
            go = row["spade"]["g_off"]
            g = data["gamma0"].to(dtype).clone()
            g[..., go:go + Cout] = gamma
            gown = torch.zeros(g.shape, dtype=torch.bool)
            gown[..., go:go + Cout] = True
            out.update(gamma_out=g, gamma_own=gown)
    else:
        if d["act"] == ACT_LEAKY:
            v = _leaky(v, d["slope"], dtype)
        elif d["act"] == ACT_TANH:
            v = torch.tanh(v)
        if data["res"] is not None:
            v = v + data["res"].to(dtype)[..., own_c]
        if data["gate"] is not None:
            gs = torch.tensor(float(torch.tensor(row["gate_slope"], dtype=torch.float32)), dtype=dtype)
            v = v * torch.where(data["gate"][..., own_c] > 0, torch.ones((), dtype=dtype), gs)      # an exact zero takes the slope
    y = data["y0"].to(dtype).clone()
    assert tuple(y.shape[:3]) == tuple(v.shape[:3]) and y.shape[3] == d["y_cs"], (y.shape, v.shape)
    y[..., own_c] = v
    own = torch.zeros(y.shape, dtype=torch.bool)
    own[..., own_c] = True
    out.update(y=y, own=own)
    return out


def wino_wgrad_ref64(row, data, dtype=torch.float64):
    """dw[o][a][b][c] = sum_pixels dy[p][o] * x[p + (a - 1, b - 1)][c] in [Cout][3][3][Cin], and db[o] = sum_pixels dy[p][o]."""
    d, xo, yo = row["d"], row["x_off"], row["y_off"]
    xs, g = data["x"].to(dtype)[..., xo:xo + d["Cin"]], data["dy"].to(dtype)[..., yo:yo + d["Cout"]]
    assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(g).all())
    B, H, W, _ = xs.shape
    xp = torch.zeros(B, H + 2, W + 2, d["Cin"], dtype=dtype)
    xp[:, 1:H + 1, 1:W + 1] = xs
    g2 = g.reshape(-1, d["Cout"])
    dw = torch.zeros(d["Cout"], 3, 3, d["Cin"], dtype=dtype)
    for a in range(3):
        for b in range(3):
            dw[:, a, b, :] = g2.t() @ xp[:, a:a + H, b:b + W].reshape(-1, d["Cin"])
    return dict(dw=dw, db=g2.sum(0) if row["db"] else None)


def reference(row, data, dtype=torch.float64):
    return wino_wgrad_ref64(row, data, dtype) if row["entry"] == "wgrad" else wino_ref64(row, data, dtype)


# ------------------------------------------------------------------------------------------------ operands
def out_size(row):
    d = row["d"]
    return (d["H"], d["W"]) if row["fam"] != "f34" else (d["H"] + 2 * row["pad"] - 3, d["W"] + 2 * row["pad"] - 3)


def shapes(row):
    """{name: shape} of what the device test allocates for the row (float32)."""
    d = row["d"]
    Ho, Wo = out_size(row)
    O, I, k, _, _ = pack_geometry(row)
    out = dict(x=(d["B"], d["H"], d["W"], d["x_cs"]))
    if row["entry"] == "wgrad":
        out.update(dy=(d["B"], d["H"], d["W"], d["y_cs"]), dw=(d["Cout"], 3, 3, d["Cin"]), db=(d["Cout"],))
        return out
    out.update(w=(O, I, k, k), y=(d["B"], Ho, Wo, d["y_cs"]), bias=(O,))
    if row["entry"] == "part" and row["part"]["mod"]:
        out.update(gamma=(d["B"], Ho, Wo, row["part"]["gamma_cs"]))
    if row["entry"] == "spade":
        out.update(gamma=(d["B"], Ho, Wo, row["spade"]["gamma_cs"]))
    return out


def _sliced(shape, off, n, g):
    """Seeded values in channels [off, off + n) of the last axis, NaN in every other."""
    t = torch.full(shape, float("nan"))
    t[..., off:off + n] = torch.randn(shape[:-1] + (n,), generator=g)
    return t


def buffers(row):
    """Seeded float32 operands of the row: NaN outside every slice a kernel may read, the sentinel in y and gamma_out."""
    g = torch.Generator().manual_seed(zlib.crc32(row["name"].encode()))
    d, sh = row["d"], shapes(row)
    xo, yo = row["x_off"], row["y_off"]
    out = dict(x=_sliced(sh["x"], xo, d["Cin"], g))
    if row["entry"] == "wgrad":
        out["dy"] = _sliced(sh["dy"], yo, d["Cout"], g)
        return out
    O, I, k, N, K = pack_geometry(row)
    out["w"] = torch.randn(sh["w"], generator=g) * (1.0 / (k * k * K)) ** 0.5
    out["sigma"] = torch.tensor([1.7]) if row["sigma"] else None
    if row["sigma"]:
        out["w"] = out["w"] * 1.7
    out["bias"] = 0.3 * torch.randn(sh["bias"], generator=g) if row["bias"] else None
    out["res"] = _sliced(sh["y"], yo, d["Cout"], g) if row["res"] else None
    out["gate"] = None
    if row["gate"]:
        gt = _sliced(sh["y"], yo, d["Cout"], g)
        zero = torch.rand(sh["y"], generator=g) < 1 / 3
        out["gate"] = torch.where(zero & torch.isfinite(gt), torch.zeros(()), gt)     # a third exact zeros, the rest of both signs
    out["y0"] = torch.full(sh["y"], SENTINEL)
    mod = (row["entry"] == "part" and row["part"]["mod"]) or row["entry"] == "spade"
    if mod:
        out["mod_x"] = _sliced(sh["y"], yo, d["Cout"], g) * 2.0 + 0.5
        out["mean"] = 0.5 + 0.2 * torch.randn(d["Cout"], generator=g)
        out["invstd"] = 0.4 + 0.2 * torch.rand(d["Cout"], generator=g)
    if row["entry"] == "part" and row["part"]["mod"]:
        out["mod_gamma"] = _sliced(sh["gamma"], row["part"]["g_off"], d["Cout"], g) * 0.5
    if row["entry"] == "spade":
        out["gamma0"] = torch.full(sh["gamma"], SENTINEL)
    return out


# ------------------------------------------------------------------------------------------------ rows
CASES = []


def _row(name, fam, entry, d, **kw):
    row = dict(name=name, fam=fam, entry=entry, d=d, pad=1, x_off=0, y_off=0, bias=False, res=False, gate=False, gate_slope=0.0,
               ws="given", wfmt="contig", sigma=False, bwd=False, db=False, part=None, spade=None, both_forms=False,
               refuse=None, how=None, cls=None)
    row.update(kw)
    if d["x_cs"] != d["Cin"] and row["refuse"] is None:
        row["x_off"] = OFF
    if d["y_cs"] != d["Cout"] and row["refuse"] is None:
        row["y_off"] = OFF
    if row["refuse"] is None:
        row["cls"] = classify(row)
    assert name not in {r["name"] for r in CASES}, name
    CASES.append(row)
    return row


def _conv(name, fam, B, H, W, Cin, Cout, xs=0, ys=0, act=ACT_NONE, slope=0.0, **kw):
    """A convolution row; xs / ys: floats by which x_cs / y_cs exceed the channel counts (the slice then starts at OFF)."""
    return _row(name, fam, kw.pop("entry", "conv"), wino_desc(B, H, W, Cin, Cout, Cin + xs, Cout + ys, act, slope), **kw)


ALL_EPI = dict(bias=True, act=ACT_LEAKY, slope=0.2, res=True, gate=True, gate_slope=0.25)


def _epilogues(prefix, fam, B, H, W, Cin, Cout, **kw):
    _conv(prefix + "_bias", fam, B, H, W, Cin, Cout, bias=True, **kw)
    _conv(prefix + "_leaky", fam, B, H, W, Cin, Cout, act=ACT_LEAKY, slope=0.2, **kw)
    _conv(prefix + "_tanh", fam, B, H, W, Cin, Cout, act=ACT_TANH, **kw)
    _conv(prefix + "_res", fam, B, H, W, Cin, Cout, res=True, **kw)
    _conv(prefix + "_gate", fam, B, H, W, Cin, Cout, gate=True, gate_slope=0.25, **kw)
    _conv(prefix + "_all", fam, B, H, W, Cin, Cout, **dict(ALL_EPI, **kw))


# ---- F(2x2,3x3): the six (TW, NTB) instantiations at one stage (Cin = 16), W in {8, 16, 32} x Cout {<= 32, > 32}
for _w in (8, 16, 32):
    _conv("f2_w%d_c32" % _w, "f2", 2, 4, _w, 16, 32)
    _conv("f2_w%d_c64" % _w, "f2", 2, 4, _w, 16, 64, bias=True)
_conv("f2_h2_one_tile_row", "f2", 1, 2, 8, 16, 8)
_conv("f2_stages2", "f2", 1, 4, 8, 32, 8)
_conv("f2_stages3_odd", "f2", 1, 4, 8, 48, 8)
# ragged regions in x and in y: W/2 no multiple of TW, H/2 no multiple of TH
_conv("f2_ragged_tw4", "f2", 1, 18, 10, 16, 8)                         # 5 x 9 tiles in regions of 4 x 8
_conv("f2_ragged_tw8", "f2", 1, 10, 18, 16, 40)                        # 9 x 5 tiles in regions of 8 x 4
_conv("f2_ragged_tw16", "f2", 1, 6, 34, 16, 8)                         # 17 x 3 tiles in regions of 16 x 2
# Cout tails (N no multiple of 32 in the pack)
_conv("f2_cout4", "f2", 2, 4, 8, 16, 4, bias=True)
_conv("f2_cout36", "f2", 2, 4, 16, 16, 36, bias=True)
_conv("f2_cout100", "f2", 1, 4, 32, 16, 100, bias=True)
_epilogues("f2_epi", "f2", 2, 6, 12, 32, 36)
# strided y, residual and gate, once per TW; and without an epilogue (the convolution entries take a dense x)
for _w in (8, 16, 32):
    _conv("f2_strided_w%d" % _w, "f2", 2, 4, _w, 16, 36, ys=12, **ALL_EPI)
_conv("f2_strided_plain", "f2", 2, 6, 12, 32, 8, ys=12)
_conv("f2_strided_y_only", "f2", 2, 6, 12, 32, 8, ys=12, res=True)
# the split over the input channels: 1 block, 16 stages -> 2 ranges of 8; 17 stages -> 9 + 8; 81 stages: ks = 10 gives 9 ranges
_conv("f2_split_min", "f2", 1, 2, 8, 256, 4)
_conv("f2_split_uneven17", "f2", 1, 2, 8, 272, 4)
_conv("f2_split_ksplit_below_ks", "f2", 1, 2, 8, 1296, 4)
_conv("f2_split_w16_c64", "f2", 1, 4, 16, 256, 64)
_conv("f2_split_strided_y_runs_unsplit", "f2", 1, 2, 8, 256, 4, ys=8)
_conv("f2_split_short_workspace", "f2", 1, 2, 8, 256, 4, ws="short")
_conv("f2_stages15_plain", "f2", 1, 2, 8, 240, 4)
# the packs: channels-last, a channel slice of a larger parameter, sigma, the backward-data operand at channel tails
_conv("f2_pack_cl", "f2", 1, 4, 8, 32, 36, wfmt="cl")
_conv("f2_pack_slice", "f2", 1, 4, 8, 32, 36, wfmt="slice")
_conv("f2_pack_sigma", "f2", 1, 4, 8, 32, 36, sigma=True)
_conv("f2_pack_bwd_tail", "f2", 1, 4, 8, 48, 20, bwd=True)              # the weight is (48, 20, 3, 3): N = 20, K = 48
_conv("f2_pack_bwd_sigma_slice", "f2", 1, 4, 16, 32, 100, bwd=True, sigma=True, wfmt="slice", gate=True, gate_slope=0.0)

# ---- F(4x4,3x3): the minimum map 16 x 32, stage counts 1 | 2 | 3 | 4, Cout 4 | 36 | 64 | 100
_conv("f4_s1_c4", "f4", 1, 16, 32, 8, 4)
_conv("f4_s2_c36", "f4", 1, 16, 32, 16, 36, bias=True)
_conv("f4_s3_c100", "f4", 1, 16, 32, 24, 100, bias=True)
_conv("f4_s4_c64", "f4", 2, 16, 32, 32, 64)
_conv("f4_s5", "f4", 1, 16, 32, 40, 8)
_conv("f4_ragged", "f4", 1, 20, 36, 16, 36)
_epilogues("f4_epi", "f4", 1, 20, 36, 16, 36)
_conv("f4_strided_plain", "f4", 1, 16, 32, 16, 36, ys=12)
_conv("f4_strided_all", "f4", 2, 20, 36, 24, 100, ys=12, **ALL_EPI)
_conv("f4_split_min", "f4", 1, 16, 32, 256, 4)
_conv("f4_split_c100", "f4", 1, 20, 36, 264, 100)                      # 33 stages: 17 + 16
_conv("f4_split_strided_y_runs_unsplit", "f4", 1, 16, 32, 256, 4, ys=8)
_conv("f4_split_short_workspace", "f4", 1, 16, 32, 256, 4, ws="short")
_conv("f4_pack_cl", "f4", 1, 16, 32, 16, 36, wfmt="cl")
_conv("f4_pack_slice_sigma", "f4", 1, 16, 32, 16, 36, wfmt="slice", sigma=True)
_conv("f4_pack_bwd_tail", "f4", 1, 16, 32, 24, 20, bwd=True)
# the persistent form: at least 2 x (CU count & ~7) items, an even stage count >= 4, Cout % 64 == 0 - 512 items on 256 CUs
_conv("f4_persist_dense", "f4", 4, 64, 128, 32, 512, both_forms=True)
_conv("f4_persist_strided", "f4", 4, 64, 128, 32, 512, ys=8, both_forms=True)
_conv("f4_persist_ragged", "f4", 4, 60, 124, 32, 512, both_forms=True)
_conv("f4_persist_all_strided", "f4", 4, 64, 128, 32, 512, ys=8, both_forms=True, **ALL_EPI)
_conv("f4_persist_odd_stages_one_item", "f4", 4, 64, 128, 24, 512)
# csg_wino4_conv_part: tiles [tile_off, tile_off + Cout / 32) of an operand of tiles_total tiles
_conv("f4_part_plain", "f4", 1, 16, 32, 16, 32, ys=12, entry="part", bias=True, part=dict(tile_off=1, tiles_total=3, mod=False))
_conv("f4_part_mod", "f4", 1, 20, 36, 16, 64, ys=12, entry="part", bias=True,
      part=dict(tile_off=1, tiles_total=3, mod=True, gamma_cs=72, g_off=OFF, mod_slope=0.2))
# csg_wino4_conv_spade: bit-identical to the conv_part pair; 64 regions x 8 (gamma tile + beta tile) blocks = 512 items
_conv("f4_spade", "f4", 4, 64, 128, 32, 256, ys=12, entry="spade", bias=True,
      spade=dict(gamma_out=False, gamma_cs=264, g_off=OFF, mod_slope=0.2))
_conv("f4_spade_gamma_out", "f4", 4, 64, 128, 32, 256, ys=12, entry="spade", bias=True,
      spade=dict(gamma_out=True, gamma_cs=264, g_off=OFF, mod_slope=0.2))

# ---- F(3x3,4x4): pad 1 | 2 on 4x4 weights
_conv("f34_pad1_2x2_to_1x1", "f34", 2, 2, 2, 8, 4, pad=1)
_conv("f34_pad2_1x1_to_2x2", "f34", 2, 1, 1, 8, 4, pad=2)              # w4_plan admits H + 2 pad >= 4
_conv("f34_pad2_7x10", "f34", 1, 6, 9, 16, 36, pad=2, bias=True)       # outputs no multiple of 3
_conv("f34_pad1_regions", "f34", 1, 15, 28, 24, 100, pad=1, bias=True)  # 13 x 26 outputs: 2 x 2 regions of 12 x 24
_epilogues("f34_epi", "f34", 1, 6, 9, 16, 36, pad=2)
_conv("f34_strided_plain", "f34", 1, 6, 9, 16, 36, ys=12, pad=2)
_conv("f34_strided_all", "f34", 2, 7, 5, 24, 100, ys=12, pad=1, **ALL_EPI)
_conv("f34_split_min", "f34", 1, 2, 2, 256, 4, pad=2)
_conv("f34_split_bwd", "f34", 1, 5, 6, 256, 36, pad=1, bwd=True)
_conv("f34_pack_bwd_tail", "f34", 1, 6, 9, 24, 20, pad=1, bwd=True)
_conv("f34_pack_slice_sigma", "f34", 1, 6, 9, 16, 36, pad=2, wfmt="slice", sigma=True)


# ---- weight gradients
def _wg(name, fam, B, H, W, Cin, Cout, xs=0, ys=0, db=False, **kw):
    return _row(name, fam, "wgrad", wino_desc(B, H, W, Cin, Cout, Cin + xs, Cout + ys), db=db, **kw)


# F(3x3,2x2): each TSX at one region per image - 8x8, 4x16, 2x32; one slice: the kernel writes dw and db itself
for _h, _w in ((8, 8), (4, 16), (2, 32)):
    _wg("wg2_%dx%d_db" % (_h, _w), "wg2", 1, _h, _w, 32, 64, db=True)
    _wg("wg2_%dx%d" % (_h, _w), "wg2", 1, _h, _w, 32, 64)
    _wg("wg2_%dx%d_b9_db" % (_h, _w), "wg2", 9, _h, _w, 32, 64, db=True)       # 9 regions: 2 slices of 5 + 4
    _wg("wg2_%dx%d_b9" % (_h, _w), "wg2", 9, _h, _w, 32, 64)
    _wg("wg2_%dx%d_strided" % (_h, _w), "wg2", 2, _h, _w, 20, 36, xs=8, ys=12, db=True)
_wg("wg2_cin20", "wg2", 2, 8, 8, 20, 64, db=True)
_wg("wg2_cout36", "wg2", 2, 8, 8, 32, 36, db=True)
_wg("wg2_cin36_cout100", "wg2", 2, 16, 16, 36, 100, db=True)
_wg("wg2_cin36_cout100_b9_strided", "wg2", 9, 8, 8, 36, 100, xs=8, ys=12)
# F(3x3,4x4): one 8x8 region; 17 regions: 2 slices of 9 + 8; always summed, two slabs per slice
_wg("wg4_one_region_db", "wg4", 1, 8, 8, 64, 64, db=True)
_wg("wg4_one_region", "wg4", 1, 8, 8, 64, 64)
_wg("wg4_b17_db", "wg4", 17, 8, 8, 64, 64, db=True)
_wg("wg4_b17", "wg4", 17, 8, 8, 64, 64)
_wg("wg4_c72_c100", "wg4", 2, 8, 16, 72, 100, db=True)
_wg("wg4_c100_c72", "wg4", 2, 16, 8, 100, 72)
_wg("wg4_strided", "wg4", 2, 8, 16, 72, 100, xs=8, ys=12, db=True)
_wg("wg4_b17_strided", "wg4", 17, 8, 8, 8, 4, xs=8, ys=12)

# ---- refusals: (code, what csg_last_error says); `how`: the argument that is wrong where the descriptor is not
_conv("refuse_f2_xcs_below_cin", "f2", 1, 4, 8, 16, 8, xs=-4, refuse=(E_UNSUPPORTED, "multiples of 4"))
_conv("refuse_f4_xcs_mod4", "f4", 1, 16, 32, 16, 8, xs=2, refuse=(E_UNSUPPORTED, "multiples of 4"))
_conv("refuse_f34_ycs_below_cout", "f34", 1, 6, 9, 16, 8, ys=-4, pad=2, refuse=(E_UNSUPPORTED, "multiples of 4"))
_conv("refuse_f2_strided_x", "f2", 1, 4, 8, 16, 8, xs=8, refuse=(E_UNSUPPORTED, "x must be dense"))
_conv("refuse_f4_strided_x", "f4", 1, 16, 32, 16, 8, xs=8, refuse=(E_UNSUPPORTED, "x must be dense"))
_conv("refuse_f34_strided_x", "f34", 1, 6, 9, 16, 8, xs=8, pad=2, refuse=(E_UNSUPPORTED, "x must be dense"))
_conv("refuse_f4_part_strided_x", "f4", 1, 16, 32, 16, 32, xs=8, entry="part", bias=True, refuse=(E_UNSUPPORTED, "x must be dense"),
      part=dict(tile_off=1, tiles_total=3, mod=False))
_conv("refuse_f4_spade_strided_x", "f4", 4, 64, 128, 32, 256, xs=8, entry="spade", bias=True, refuse=(E_UNSUPPORTED, "x must be dense"),
      spade=dict(gamma_out=False, gamma_cs=256, g_off=0, mod_slope=0.2))
_conv("refuse_f2_cin24", "f2", 1, 4, 8, 24, 8, refuse=(E_UNSUPPORTED, "multiple of 16"))
_conv("refuse_f4_cin12", "f4", 1, 16, 32, 12, 8, refuse=(E_UNSUPPORTED, "multiple of 8"))
_conv("refuse_f2_misaligned_x", "f2", 1, 4, 8, 16, 8, refuse=(E_UNSUPPORTED, "16-byte aligned"), how="x")
_conv("refuse_f4_misaligned_y", "f4", 1, 16, 32, 16, 8, refuse=(E_UNSUPPORTED, "16-byte aligned"), how="y")
_conv("refuse_f34_misaligned_packed", "f34", 1, 6, 9, 16, 8, pad=2, refuse=(E_UNSUPPORTED, "16-byte aligned"), how="packed")
_conv("refuse_f2_pack_misaligned", "f2", 1, 4, 8, 16, 8, refuse=(E_UNSUPPORTED, "packed must be 16-byte aligned"), how="pack")
_conv("refuse_f4_pack_misaligned", "f4", 1, 16, 32, 16, 8, refuse=(E_UNSUPPORTED, "packed must be 16-byte aligned"), how="pack")
_wg("refuse_wg2_short_workspace", "wg2", 9, 8, 8, 32, 64, db=True, refuse=(E_WORKSPACE, "workspace"), how="short")
_wg("refuse_wg2_direct_short_workspace", "wg2", 1, 8, 8, 32, 64, refuse=(E_WORKSPACE, "workspace"), how="short")
_wg("refuse_wg4_short_workspace", "wg4", 1, 8, 8, 64, 64, db=True, refuse=(E_WORKSPACE, "workspace"), how="short")
_conv("refuse_f4_part_tiles", "f4", 1, 16, 32, 16, 64, entry="part", bias=True, refuse=(E_BADSHAPE, r"tiles \[1, 3\) of 2"),
      part=dict(tile_off=1, tiles_total=2, mod=False))
_conv("refuse_f4_spade_unqualified", "f4", 1, 16, 32, 32, 64, entry="spade", bias=True, refuse=(E_UNSUPPORTED, "does not qualify"),
      spade=dict(gamma_out=False, gamma_cs=64, g_off=0, mod_slope=0.2))

# pack-only rows: (family, O, I) with K = I no multiple of 8 (no convolution admits it) and N = O no multiple of 32.  The
# packed buffer starts as NaN; the pack of the weight zero-padded to (32, 16) must equal it bit for bit.
PACK_TAILS = (("f2", 20, 12), ("f4", 20, 12), ("f34", 20, 12), ("f2", 36, 4), ("f4", 4, 20))


def safe_row(row):
    """A refusal row with strides its buffers can be allocated with (the refused descriptor itself stays in row["d"])."""
    d = row["d"]
    up4 = lambda v: (v + 3) // 4 * 4
    return dict(row, d=dict(d, x_cs=max(up4(d["x_cs"]), d["Cin"]), y_cs=max(up4(d["y_cs"]), d["Cout"])))


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]
