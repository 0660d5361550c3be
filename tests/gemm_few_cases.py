"""The GEMM and few-output matrix: one row per LAUNCH RULE of csrc/gemm.hip (k_gemm_nt, k_gemm_tn) and csrc/fewn.hip
(k_few_fwd, k_few_finish, k_few_bwd_data, k_few_bwd_weight) and of the slab sum behind them (csrc/csg_reduce.h).

Three things live here, all host-side and (but for the ctypes structs) free of the package:

* the launch rules restated in Python from the host side of the two files - `nt_plan` (tile 128 x 64 | 128 x 128, BK 32 | 16,
  stages, grid), `xcd_remap`, `tn_plan` (row slices), `few_fwd_plan` (TX, channel split, the finish loop), `few_bwd_plan`
  (pixel lanes, pixels per block, the output-pixel partition of db), `slab_sum_form`, and the workspace bytes that follow.
  tests/test_gemm_few_cases.py holds them to the library's own workspace queries;
* float64 references from the row alone (`nt_ref`, `tn_ref`, `few_ref`, each taking a dtype, so the float32 CPU
  evaluation of the same restatement exists for the band rule of the device test);
* `CASES`: the rows, `REFUSALS`: calls the library must refuse, `ENTRY_CASES`: two rows through `ops`.

Data (`make_data(row, kind)`), seeded from the row's name.  "random": randn operands, weights scaled by 1 / sqrt(terms).
"exact": every operand a small integer in [-2, 2], slopes 0.25 | 0.5, tanh rows with act = none - every partial sum stays
below 2^24 (`exact_bound`), so every fp32 result is exact in any order of summation and the device must EQUAL the float64
reference.  Gates are drawn from {-1.5, -0.0, 0.0, 0.5, randn}, a third of them exact zeros of either sign.  What the kernels
must not read holds NaN: the pad columns of every row stride, channels [Cin, x_cs) of x, rows [cout_real, 4) of the few-output
weights and bias.  dy of the few-output rows carries 0.75 in its pad channels: dw and db must hold zeros beyond cout_real
whatever the caller left there (include/csg_hip.h)."""
import zlib

import torch
import torch.nn.functional as F

ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
SENTINEL = -3.25
DY_PAD = 0.75
FW_CK = 16
NAN = float("nan")


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ the launch rules, restated
def nt_supported(M, N, K, lda, ldb, ldy):
    """nt_ok of csrc/gemm.hip."""
    return (M > 0 and N > 0 and K > 0 and K % 4 == 0 and N % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and ldy % 4 == 0
            and lda >= K and ldb >= K and ldy >= N and 128 * lda * 4 < 2 ** 30 and 128 * ldb * 4 < 2 ** 30
            and M < 2 ** 31 - 128 and N < 2 ** 31 - 128 and cdiv(M, 128) * cdiv(N, 128) < 2 ** 31)


def nt_plan(M, N, K):
    narrow = N <= 64
    tile, bk = (64, 32) if narrow else (128, 16)
    return dict(narrow=narrow, tile=tile, bk=bk, nstage=cdiv(K, bk), nnb=cdiv(N, tile), grid=cdiv(M, 128) * cdiv(N, tile),
                tail_slots=(K % bk) // 4)


def xcd_remap(bid, nblk):
    """gm_xcd_remap: the logical tile of hardware block `bid` of `nblk`."""
    q, r = nblk >> 3, nblk & 7
    xcd, idx = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def tn_plan(M, N, K):
    tiles = cdiv(N, 128) * cdiv(K, 128)
    want = max(1, min(cdiv(1024, tiles), max(M // 256, 1)))
    per = cdiv(cdiv(M, want), 32) * 32
    ns = cdiv(M, per)
    last = M - (ns - 1) * per
    return dict(nsplit=ns, rows_per=per, last_rows=last, stages=cdiv(min(per, M), 16), last_stages=cdiv(last, 16),
                last_stage_rows=last - (cdiv(last, 16) - 1) * 16, tiles=tiles, direct=ns == 1,
                ws_bytes=ns * (N * K + N) * 4 if ns > 1 else 0)


def slab_sum_form(nslabs):
    return "wide" if nslabs >= 16 else "narrow"


def few_supported(d):
    """few_plan of csrc/fewn.hip: None, or the text the refusal carries."""
    if not ((d["KH"] == 3 and d["KW"] == 3) or (d["KH"] == 4 and d["KW"] == 4)):
        return "only 3x3 and 4x4 kernels"
    if not (d["Cin"] % 32 == 0 and d["Cin"] <= 1024 and 1024 % d["Cin"] == 0 and d["x_cs"] % 4 == 0 and d["x_cs"] >= d["Cin"]):
        return r"must be 32, 64, \.\.\., 1024"
    if not 1 <= d["cout_real"] <= 4:
        return r"1\.\.4 output channels"
    if d["KH"] * d["KW"] * d["cout_real"] > 36:
        return "do not fit the registers"
    if few_out(d)[0] <= 0 or few_out(d)[1] <= 0:
        return "empty output"
    return None


def few_out(d):
    return d["IH"] + 2 * d["pad"] - d["KH"] + 1, d["IW"] + 2 * d["pad"] - d["KW"] + 1


def few_fwd_plan(d):
    OH, OW = few_out(d)
    TX = 32 if OW > 48 else 16
    TY = 256 // TX
    tiles = d["B"] * cdiv(OH, TY) * cdiv(OW, TX)
    nchunk = d["Cin"] // FW_CK
    ks = min(cdiv(1536, tiles) if tiles < 1024 else 1, nchunk)
    cps = cdiv(nchunk, ks)
    ksplit = cdiv(nchunk, cps)
    slab = d["B"] * OH * OW * 4
    return dict(TX=TX, TY=TY, tiles=tiles, nchunk=nchunk, cps=cps, ksplit=ksplit, last_chunks=nchunk - (ksplit - 1) * cps,
                fours=(ksplit - 1) // 4, rem=(ksplit - 1) % 4, ragged=bool(OH % TY or OW % TX),
                ws_bytes=ksplit * slab * 4 if ksplit > 1 else 0)


def few_bwd_plan(d):
    OH, OW = few_out(d)
    npix, nout = d["B"] * d["IH"] * d["IW"], d["B"] * OH * OW
    PL = 256 // (d["Cin"] // 4)
    ppb = cdiv(max(cdiv(npix, 1024), 32 * PL), PL) * PL
    blocks = cdiv(npix, ppb)
    return dict(PL=PL, ppb=ppb, blocks=blocks, last_pixels=npix - (blocks - 1) * ppb, opb=cdiv(nout, blocks), npix=npix, nout=nout,
                ws_bytes=blocks * (4 * d["KH"] * d["KW"] * d["Cin"] + 4) * 4)


# ------------------------------------------------------------------------------------------------ launch classes
def _stage_kind(K, bk):
    n = cdiv(K, bk)
    if n == 1:
        return "1 partial" if K % bk else "1 full"
    if n == 2:
        return "2 with tail" if K % bk else "2"
    return "odd" if n % 2 else "even"


def nt_class(r):
    p = nt_plan(r["M"], r["N"], r["K"])
    return (p["tile"], "gated" if r["gated"] else "plain", _stage_kind(r["K"], p["bk"]))


def tn_class(r):
    p = tn_plan(r["M"], r["N"], r["K"])
    form = "direct" if p["direct"] else slab_sum_form(p["nsplit"])
    return (form, "db" if r["db"] else "nodb", "tails" if r["N"] % 128 or r["K"] % 128 else "whole")


def few_fwd_class(r):
    """(TX, how the channels are cut, the finish loop, (kernel side, outputs) = the template instance)."""
    d, p = r["desc"], few_fwd_plan(r["desc"])
    if r["ws"] != "full" and p["ksplit"] > 1:
        cut, fin = "refused", "none"
    elif p["ksplit"] == 1:
        cut, fin = "unsplit", "none"
    else:
        cut = "uneven" if p["last_chunks"] != p["cps"] else "even"
        fin = ("fours + remainder" if p["rem"] else "fours") if p["fours"] else "remainder"
    return (p["TX"], cut, fin, (d["KH"], d["cout_real"]))


def few_bwd_class(r):
    """(PL, one | many blocks, a step of PL pixels against a row and an image, the slab sum's form)."""
    d, p = r["desc"], few_bwd_plan(r["desc"])
    step = "image" if p["PL"] > d["IH"] * d["IW"] else ("row" if p["PL"] > d["IW"] else "in row")
    return (p["PL"], "one" if p["blocks"] == 1 else "many", step, slab_sum_form(p["blocks"]))


def describe(r):
    if r["kind"] == "nt":
        p = nt_plan(r["M"], r["N"], r["K"])
        return "nt %dx%dx%d tile %d bk %d stages %d (tail %d slots) grid %d%s" % (
            r["M"], r["N"], r["K"], p["tile"], p["bk"], p["nstage"], p["tail_slots"], p["grid"], " gated" if r["gated"] else "")
    if r["kind"] == "tn":
        p = tn_plan(r["M"], r["N"], r["K"])
        return "tn %dx%dx%d %s nsplit %d rows_per %d last %d%s" % (
            r["M"], r["N"], r["K"], tn_class(r)[0], p["nsplit"], p["rows_per"], p["last_rows"], " db" if r["db"] else "")
    f, b = few_fwd_plan(r["desc"]), few_bwd_plan(r["desc"])
    return "few TX %d tiles %d cps %d ksplit %d (%s) | PL %d ppb %d blocks %d last %d opb %d" % (
        f["TX"], f["tiles"], f["cps"], f["ksplit"], few_fwd_class(r)[1], b["PL"], b["ppb"], b["blocks"], b["last_pixels"], b["opb"])


# ------------------------------------------------------------------------------------------------ rows
CASES = []


def _add(row):
    assert row["name"] not in {r["name"] for r in CASES}, row["name"]
    CASES.append(row)
    return row


def _nt(name, M, N, K, pads=False, bias=False, act=ACT_NONE, slope=0.0, gated=False):
    """Row strides: dense, or (pads) lda, ldb, ldy, ldg = K + 4, K + 8, N + 12, N + 16."""
    pa, pb, py, pg = (4, 8, 12, 16) if pads else (0, 0, 0, 0)
    return _add(dict(name=name, kind="nt", M=M, N=N, K=K, lda=K + pa, ldb=K + pb, ldy=N + py, ldg=N + pg, bias=bias, act=act,
                     slope=slope, gated=gated, gate_slope=0.5))


def _tn(name, M, N, K, db=True, pads=False):
    py, px = (8, 4) if pads else (0, 0)
    return _add(dict(name=name, kind="tn", M=M, N=N, K=K, ldy=N + py, ldx=K + px, db=db))


def few_desc(B, IH, IW, Cin, K, pad, cout_real, x_cs=None, act=ACT_NONE, slope=0.0, in_act=0, in_slope=0.0, KW=None):
    return dict(B=B, IH=IH, IW=IW, Cin=Cin, x_cs=Cin if x_cs is None else x_cs, KH=K, KW=K if KW is None else KW, pad=pad,
                cout_real=cout_real, act=act, slope=slope, in_act=in_act, in_slope=in_slope)


def _few(name, B, IH, IW, Cin, K, pad, cout_real, bias=True, ws="full", dirs=("fwd", "dx", "wgrad"), **kw):
    """ws: "full" (what the query asks for) | "none" | "short" (4 bytes less) for the forward's workspace."""
    return _add(dict(name=name, kind="few", desc=few_desc(B, IH, IW, Cin, K, pad, cout_real, **kw), bias=bias, ws=ws, dirs=dirs))


_nt("nt_one", 1, 4, 4)
_nt("nt_narrow_exact", 128, 64, 32, bias=True, act=ACT_LEAKY)
_nt("nt_narrow_tail", 129, 60, 36, pads=True, bias=True, act=ACT_LEAKY, slope=0.25, gated=True)
_nt("nt_narrow_odd", 300, 64, 96, gated=True)
_nt("nt_narrow_long", 64, 8, 1152)
_nt("nt_wide_first", 130, 68, 16)
_nt("nt_wide_tail", 257, 132, 20, pads=True, bias=True, act=ACT_LEAKY, slope=0.25, gated=True)
_nt("nt_wide_odd", 127, 128, 48, gated=True)
_nt("nt_wide_grid9", 1100, 128, 64, bias=True, act=ACT_LEAKY, gated=True)
_nt("nt_wide_grid17", 2100, 128, 4)
_nt("nt_wide_long", 64, 256, 1152)

_tn("tn_one_row", 1, 4, 4, db=False)
_tn("tn_17_rows", 17, 132, 4, pads=True)
_tn("tn_k_tiles", 511, 4, 260)
_tn("tn_two", 520, 8, 8)
_tn("tn_two_ragged", 700, 132, 260, pads=True)
_tn("tn_four", 1030, 256, 128, db=False)
_tn("tn_15", 4100, 4, 4)
_tn("tn_16", 4096, 4, 4)
_tn("tn_17", 4352, 4, 8)
_tn("tn_29", 8200, 132, 4)

_few("few_tiny", 3, 5, 5, 32, 3, 1, 4, act=ACT_TANH)
_few("few_1024", 2, 7, 7, 1024, 3, 0, 1)
_few("few_4x4_32", 1, 33, 33, 32, 4, 2, 2, bias=False)
_few("few_head", 2, 18, 18, 512, 4, 2, 1)
_few("few_ow49", 1, 9, 49, 64, 3, 1, 3, act=ACT_TANH, in_act=1, in_slope=0.2)
_few("few_ow48", 1, 8, 48, 64, 3, 1, 3, act=ACT_LEAKY, slope=0.25)               # leaky in place of conv_img's tanh
_few("few_ow48_4x4", 1, 17, 47, 128, 4, 2, 1)
_few("few_uneven", 300, 4, 4, 1024, 3, 1, 2)
_few("few_unsplit", 1100, 3, 3, 64, 3, 1, 3, act=ACT_TANH)
_few("few_split4", 400, 5, 5, 128, 3, 1, 1)
_few("few_bigpad", 2, 6, 10, 256, 3, 3, 3)
_few("few_wide_map", 1, 40, 600, 32, 3, 1, 3, act=ACT_TANH)
# variants: a channel slice of a wider x, every template instance, a refused forward workspace
_few("few_head_xcs", 2, 18, 18, 512, 4, 2, 1, x_cs=520)
_few("few_ow49_xcs", 1, 9, 49, 64, 3, 1, 3, x_cs=72, act=ACT_TANH, in_act=1, in_slope=0.2)
for _n in (1, 2, 3):
    _few("few_tiny_n%d" % _n, 3, 5, 5, 32, 3, 1, _n, act=ACT_TANH)
_few("few_4x4_32_n1", 1, 33, 33, 32, 4, 2, 1)
_few("few_head_no_ws", 2, 18, 18, 512, 4, 2, 1, ws="none", dirs=("fwd",))
_few("few_head_short_ws", 2, 18, 18, 512, 4, 2, 1, ws="short", dirs=("fwd",))
SPLIT_TWIN = {"few_head_no_ws": "few_head", "few_head_short_ws": "few_head"}      # the same data, split: within the gate of it

# calls the library must refuse: (name, entry, arguments, what the error text says)
REFUSALS = [
    dict(name="refuse_nt_k6", entry="nt", M=8, N=8, K=6, lda=8, ldb=8, ldy=8, ldg=8, gated=False, text="multiples of 4"),
    dict(name="refuse_nt_lda", entry="nt", M=8, N=8, K=8, lda=4, ldb=8, ldy=8, ldg=8, gated=False, text="lda/ldb >= K"),
    dict(name="refuse_nt_ldg", entry="nt", M=8, N=8, K=8, lda=8, ldb=8, ldy=8, ldg=4, gated=True, text="ldg < N"),
    dict(name="refuse_tn_short_ws", entry="tn", M=520, N=8, K=8, text=r"workspace of \d+ bytes needed"),
    dict(name="refuse_few_5x5", entry="few_fwd", desc=few_desc(1, 8, 8, 32, 5, 2, 1), text="only 3x3 and 4x4 kernels"),
    dict(name="refuse_few_cin96", entry="few_fwd", desc=few_desc(1, 8, 8, 96, 3, 1, 1), text=r"must be 32, 64, \.\.\., 1024"),
    dict(name="refuse_few_4x4_n3", entry="few_fwd", desc=few_desc(1, 8, 8, 32, 4, 2, 3), text="do not fit the registers"),
    dict(name="refuse_few_wgrad_short_ws", entry="few_wgrad", desc=few_desc(2, 18, 18, 512, 4, 2, 1), text=r"needs \d+ bytes"),
]

# through `ops`, the model's call path, with ops.GEMM_MODE = "all" and ops.GEMM_MIN_TILES = 1; `calls`: launches of gemm.hip
ENTRY_CASES = [
    dict(name="entry_linear_relu_linear", kind="linear", M=257, dims=(36, 132, 64), calls=6),
    dict(name="entry_conv1x1", kind="conv1x1", B=2, H=9, W=13, Cin=64, Cout=68, calls=3),
]
KINK_CLEARANCE = 1e-4
KINDS = ("random", "exact")


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


def by_name(name):
    (c,) = [c for c in CASES + REFUSALS + ENTRY_CASES if c["name"] == name]
    return c


def few_to_ctypes(d):
    from canonicalsg2im_amd._lib import FewDesc
    cd = FewDesc()
    for k, v in d.items():
        setattr(cd, k, v)
    return cd


def nt_to_ctypes(r):
    from canonicalsg2im_amd._lib import GemmDesc
    cd = GemmDesc()
    cd.M, cd.N, cd.K, cd.lda, cd.ldb, cd.ldy, cd.ldg = r["M"], r["N"], r["K"], r["lda"], r["ldb"], r["ldy"], r["ldg"]
    cd.act, cd.slope, cd.gate_slope = r.get("act", ACT_NONE), r.get("slope", 0.0), r.get("gate_slope", 0.5)
    return cd


# ------------------------------------------------------------------------------------------------ operands
def buffers(r):
    """{name: shape} of what the device test allocates for the row (float32); tests/test_gemm_few_cases.py checks on the CPU
    that every address the kernels can form from the row lies inside."""
    if r["kind"] == "nt":
        return dict(a=(r["M"], r["lda"]), bw=(r["N"], r["ldb"]), bias=(r["N"],), gate=(r["M"], r["ldg"]), y=(r["M"], r["ldy"]))
    if r["kind"] == "tn":
        return dict(dy=(r["M"], r["ldy"]), x=(r["M"], r["ldx"]), dw=(r["N"], r["K"]), db=(r["N"],),
                    ws=(tn_plan(r["M"], r["N"], r["K"])["ws_bytes"] // 4,))
    d = r["desc"]
    OH, OW = few_out(d)
    return dict(x=(d["B"], d["IH"], d["IW"], d["x_cs"]), w=(4, d["KH"], d["KW"], d["Cin"]), bias=(4,), y=(d["B"], OH, OW, 4),
                dy=(d["B"], OH, OW, 4), dx=(d["B"], d["IH"], d["IW"], d["x_cs"]), dw=(4, d["KH"], d["KW"], d["Cin"]), db=(4,),
                ws_fwd=(few_fwd_plan(d)["ws_bytes"] // 4,), ws_wgrad=(few_bwd_plan(d)["ws_bytes"] // 4,))


def _gen(name, kind):
    return torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (name, kind)).encode()))


def _draw(shape, g, kind, scale=1.0):
    if kind == "exact":
        return torch.randint(-2, 3, shape, generator=g).float()
    return torch.randn(shape, generator=g) * scale


def _gates(shape, g):
    pick = torch.randint(0, 6, shape, generator=g)
    out = torch.randn(shape, generator=g)
    for i, v in enumerate((-1.5, -0.0, 0.0, 0.5)):
        out = torch.where(pick == i, torch.full((), v), out)
    return out


def exact_slope(s):
    """The slope the exact pass runs with: 0 stays (ReLU), anything else becomes a power of two."""
    return 0.0 if s == 0 else (0.25 if s == 0.25 else 0.5)


def row_for(r, kind):
    """The row as the `kind` pass launches it: the exact pass turns tanh off and takes power-of-two slopes."""
    if kind != "exact":
        return r
    if r["kind"] == "nt":
        return dict(r, slope=exact_slope(r["slope"]))
    if r["kind"] == "few":
        d = r["desc"]
        return dict(r, desc=dict(d, act=ACT_NONE if d["act"] == ACT_TANH else d["act"], slope=exact_slope(d["slope"]),
                                 in_slope=exact_slope(d["in_slope"])))
    return r


def make_data(r, kind):
    """Seeded float32 operands of the row, NaN where no kernel may read (see the module's docstring)."""
    g = _gen(SPLIT_TWIN.get(r["name"], r["name"]), kind)
    s = buffers(r)
    if r["kind"] == "nt":
        M, N, K = r["M"], r["N"], r["K"]
        a, bw = torch.full(s["a"], NAN), torch.full(s["bw"], NAN)
        a[:, :K], bw[:, :K] = _draw((M, K), g, kind), _draw((N, K), g, kind, K ** -0.5)
        out = dict(a=a, bw=bw, bias=_draw(s["bias"], g, kind, 0.3) if r["bias"] else None, gate=None)
        if r["gated"]:
            out["gate"] = torch.full(s["gate"], NAN)
            out["gate"][:, :N] = _gates((M, N), g)
        return out
    if r["kind"] == "tn":
        dy, x = torch.full(s["dy"], NAN), torch.full(s["x"], NAN)
        dy[:, :r["N"]], x[:, :r["K"]] = _draw((r["M"], r["N"]), g, kind), _draw((r["M"], r["K"]), g, kind)
        return dict(dy=dy, x=x)
    d = r["desc"]
    x, w, bias = torch.full(s["x"], NAN), torch.full(s["w"], NAN), torch.full(s["bias"], NAN)
    x[..., :d["Cin"]] = _draw(s["x"][:3] + (d["Cin"],), g, kind)
    w[:d["cout_real"]] = _draw((d["cout_real"],) + s["w"][1:], g, kind, (d["KH"] * d["KW"] * d["Cin"]) ** -0.5)
    bias[:d["cout_real"]] = _draw((d["cout_real"],), g, kind, 0.3)
    dy = torch.full(s["dy"], DY_PAD)
    dy[..., :d["cout_real"]] = _draw(s["dy"][:3] + (d["cout_real"],), g, kind)
    return dict(x=x, w=w, bias=bias if r["bias"] else None, dy=dy)


def exact_bound(r):
    """The largest magnitude any partial sum of the exact pass can reach, in any order (operands in [-2, 2])."""
    if r["kind"] == "nt":
        return 4 * r["K"] + 2
    if r["kind"] == "tn":
        return 4 * r["M"]
    d = r["desc"]
    OH, OW = few_out(d)
    return max(4 * d["KH"] * d["KW"] * d["Cin"] + 2, 4 * d["B"] * d["IH"] * d["IW"], 2 * d["B"] * OH * OW, 4 * d["KH"] * d["KW"] * 4)


# ------------------------------------------------------------------------------------------------ the contract in float64
def _leaky(v, slope):
    return torch.where(v > 0, v, v * float(torch.tensor(slope, dtype=torch.float32)))          # the C field is a float


def nt_ref(r, data, dtype=torch.float64):
    """{"y": (M, N)}: a[:, :K] @ bw[:, :K].T + bias, then leaky, then * where(gate > 0, 1, gate_slope)."""
    M, N, K = r["M"], r["N"], r["K"]
    v = data["a"][:, :K].to(dtype) @ data["bw"][:, :K].to(dtype).t()
    if data["bias"] is not None:
        v = v + data["bias"].to(dtype)
    if r["act"] == ACT_LEAKY:
        v = _leaky(v, r["slope"])
    if data["gate"] is not None:
        v = v * torch.where(data["gate"][:, :N] > 0, 1.0, float(torch.tensor(r["gate_slope"], dtype=torch.float32))).to(dtype)
    return dict(y=v)


def tn_ref(r, data, dtype=torch.float64):
    dy, x = data["dy"][:, :r["N"]].to(dtype), data["x"][:, :r["K"]].to(dtype)
    return dict(dw=dy.t() @ x, db=dy.sum(0) if r["db"] else None)


def few_ref(r, data, dtype=torch.float64):
    """y (B, OH, OW, 4), dx (B, IH, IW, Cin), dw (4, KH, KW, Cin), db (4,) of the few-output row: torch's conv2d and its
    autograd on leaky(x[..., :Cin], in_slope) when in_act is set.  Rows [cout_real, 4) of every padded tensor are zero.
    dx is the gradient of the convolution's INPUT (the in_act derivative is the caller's, include/csg_hip.h)."""
    d, n = r["desc"], r["desc"]["cout_real"]
    xin = data["x"][..., :d["Cin"]].to(dtype).permute(0, 3, 1, 2)
    if d["in_act"]:
        xin = _leaky(xin, d["in_slope"])
    xin = xin.clone().requires_grad_(True)
    w = data["w"][:n].to(dtype).permute(0, 3, 1, 2).clone().requires_grad_(True)
    b = data["bias"][:n].to(dtype).clone().requires_grad_(True) if data["bias"] is not None else None
    pre = F.conv2d(xin, w, b, 1, d["pad"])
    y = pre
    if d["act"] == ACT_LEAKY:
        y = _leaky(pre, d["slope"])
    elif d["act"] == ACT_TANH:
        y = torch.tanh(pre)
    gy = data["dy"][..., :n].to(dtype).permute(0, 3, 1, 2)
    grads = torch.autograd.grad(pre, [xin, w] + ([b] if b is not None else []), gy)             # dy is the PRE-activation's
    db = grads[2] if b is not None else gy.sum((0, 2, 3))
    return dict(y=F.pad(y.detach().permute(0, 2, 3, 1), (0, 4 - n)), dx=grads[0].permute(0, 2, 3, 1).contiguous(),
                dw=F.pad(grads[1].permute(0, 2, 3, 1), (0, 0, 0, 0, 0, 0, 0, 4 - n)), db=F.pad(db, (0, 4 - n)))


def reference(r, data, dtype=torch.float64):
    return {"nt": nt_ref, "tn": tn_ref, "few": few_ref}[r["kind"]](r, data, dtype)


# ------------------------------------------------------------------------------------------------ the entry rows
def entry_data(e, kind):
    """CPU float32 operands of an entry row.  The random linear row tries seeds (row name, attempt) until the hidden
    pre-activations keep KINK_CLEARANCE clear of zero in float32 and float64: both references then take the same gates as
    the kernels and nothing has to be masked.  (The exact pass needs none of that: ReLU and its gate agree at integers.)"""
    for attempt in range(200):
        g = _gen("%s/%d" % (e["name"], attempt), kind)
        if e["kind"] == "linear":
            k0, k1, k2 = e["dims"]
            out = dict(x=_draw((e["M"], k0), g, kind), w1=_draw((k1, k0), g, kind, k0 ** -0.5), b1=_draw((k1,), g, kind, 0.3),
                       w2=_draw((k2, k1), g, kind, k1 ** -0.5), b2=_draw((k2,), g, kind, 0.3), gy=_draw((e["M"], k2), g, kind))
            if kind == "exact" or entry_clearance(out) >= KINK_CLEARANCE:
                return out
        else:
            return dict(x=_draw((e["B"], e["Cin"], e["H"], e["W"]), g, kind),
                        w=_draw((e["Cout"], e["Cin"], 1, 1), g, kind, e["Cin"] ** -0.5),
                        gy=_draw((e["B"], e["Cout"], e["H"], e["W"]), g, kind))
    raise AssertionError("no seed keeps the hidden layer clear of the kink")


def entry_clearance(data):
    """The smallest |hidden pre-activation| of the linear row, the smaller of its float32 and float64 evaluations."""
    return min(float(F.linear(data["x"].to(t), data["w1"].to(t), data["b1"].to(t)).abs().min()) for t in (torch.float32, torch.float64))


def entry_ref(e, data, dtype=torch.float64):
    """Outputs and gradients of the entry row by torch autograd in `dtype`: linear (y, dx, dw1, db1, dw2, db2); conv1x1 (y,
    dx, dw)."""
    if e["kind"] == "linear":
        leaves = [data[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2")]
        y = F.linear(F.relu(F.linear(leaves[0], leaves[1], leaves[2])), leaves[3], leaves[4])
        names = ("dx", "dw1", "db1", "dw2", "db2")
    else:
        leaves = [data[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w")]
        y = F.conv2d(leaves[0], leaves[1])
        names = ("dx", "dw")
    grads = torch.autograd.grad(y, leaves, data["gy"].to(dtype))
    return dict(zip(("y",) + names, (y.detach(),) + grads))
