"""The spectral-norm / loss / resampling path matrix: one row per code path (and per kernel corner) of csrc/spectral.hip,
csrc/perceptual.hip and the resampling kernels at the end of csrc/norm.hip that the public entry points can reach, with
`ref64`, a plain float64 CPU restatement of each contract (torch/nn/utils/spectral_norm.py `compute_weight`; reference
spade/models/networks/loss.py:60-117; nn.MaxPool2d(2, 2), nn.AvgPool2d(2, 2), nn.AvgPool2d(3, 2, 1, count_include_pad=
False), nearest F.interpolate).  Used by tests/test_gpu_loss_paths.py (each row through the entry point it names on the
device) and tests/test_loss_cases.py (on the CPU: the restatement against torch's own operators and the oracle, the
table's coverage computed from the restated launch rules, the rows' distance from every discontinuity).

A row (dict, built by `row`) holds
  name, family    — the id; "spectral" | "loss" | "resample"
  entry           — "spectral_weight" | "spectral_weights" | "l1_mean" | "gan_hinge" (GANLoss('hinge'), so that the dispatch
                    to ops.hinge_mean is part of the row) | "maxpool2" | "avgpool2" | "upsample2x" | "avgpool3s2" |
                    "pool_fanout" | "nearest_resize" (ops.*)
  shape           — spectral: the weight; l1 / resample: the (B, C, H, W) operand
  cot, scale      — spectral: the cotangent's memory layout (COTS) and what the weight is multiplied by
  members, nograd, skip_bwd — spectral_weights: the rows whose weights go into the one call; which of them does not require
                    grad; whose output stays out of the backward
  fmt             — l1: "nchw" | "nhwc"
  kind, maps      — hinge: the term (0 generator, 1 discriminator real, 2 discriminator fake) and [(shape, "pad" | "contig")]
                    per scale: channel 0 of a padded NHWC buffer of 4 channels (element stride 4) or a contiguous map
  gout            — the upstream gradient (the loss is multiplied by it before .backward())
  mode            — pool_fanout: which outputs have a consumer, "both" | "full" | "pool"
  out_size        — nearest_resize: (OH, OW)
  data            — the data recipe: "randn" | "neg" (all negative) | "ties" (few distinct values, many zeros) | "nan" (one
                    NaN) | "zeros" (l1: a block where a == b exactly) | "tie" (hinge: every third prediction on the margin)
  need            — what requires grad: ("w",) | ("a",) | ("x",) | ()
  refuse, refuse_at — the call must raise a RuntimeError matching this pattern before any launch ("fwd" | "bwd")
  seed            — added to the data generator's seed (crc32 of the name): moved when the fp64 reference alone finds the
                    row too close to a discontinuity (tests/test_loss_cases.py: conditions (a), (b), (c))

No row excludes anything from its comparison.  The one judgement that is not a distance to `ref64` is the hinge gradient
exactly ON the margin (rows with data == "tie"): every value in [0, 1] x the off-margin gradient is a subgradient there
(the kernel's documented choice is 0, torch.clamp's 1, torch.min's 1/2), so those entries are held to that interval."""
import zlib

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------- the launch rules
EW_BLOCK, EW_CAP = 256, 256 * 16     # ew_grid: csrc/perceptual.hip:123-128 and csrc/norm.hip:544-549
SN_MAXT = 12                         # csrc/spectral.hip:215: weights per launch
SN_BWD_MAXK = 15360                  # csrc/spectral.hip:367: one LDS row of the backward
SN_T_BYTES = 64 * 1024               # csrc/spectral.hip:328 and ops.py:894-895: the channels-last transpose buffer
SN_SCALE_CAP = 2048                  # csrc/spectral.hip:323-333: blocks of k_sn_scale_m per weight
SN_EPS = 1e-12                       # ops.py:971: spectral_weight's default, torch.nn.utils.spectral_norm's too
HINGE_MAX_SCALES = 4                 # ops.py:1970
COTS = ("contig", "ohwi", "ohiw", "padslice", "colmajor")


def cdiv(a, b):
    return -(-a // b)


def ew_grid(n):
    """Blocks of 256 lanes an elementwise launch over n items gets (perceptual.hip:123-128, norm.hip:544-549)."""
    return min(max(cdiv(n, EW_BLOCK), 1), EW_CAP)


def ew_capped(n):
    """The grid-stride loop takes a further trip because of the cap: more than 1,048,576 items."""
    return cdiv(n, EW_BLOCK) > EW_CAP


def sn_dims(shape):
    """(Cout, Cin, KH, KW, K) as _SpectralWeight.backward sees a weight (ops.py:924-926)."""
    Cout = shape[0]
    K = int(np.prod(shape[1:]))
    Cin, KH, KW = (shape[1], shape[2], shape[3]) if len(shape) == 4 else (K, 1, 1)
    return Cout, Cin, KH, KW, K


def sn_R(Cout, K):
    """Row chunks of the first stage of W^T u (csrc/spectral.hip:274-281)."""
    return max(min(512 // cdiv(K, 1024), Cout, 32), 1)


def sn_empty_chunks(Cout, K):
    """Chunks that hold no row and must still write zeros: per = ceil(Cout / R) (csrc/spectral.hip:41-42)."""
    R = sn_R(Cout, K)
    per = cdiv(Cout, R)
    return sum(1 for r in range(R) if r * per >= Cout)


def sn_channels_last(shape):
    """Cin if W_eff comes out in channels-last memory, else 0 (_SpectralWeight.forward, ops.py:894-895)."""
    if len(shape) == 4 and shape[1] % 4 == 0 and shape[2] * shape[3] > 1 and shape[2] * shape[3] * (shape[1] + 4) * 4 <= SN_T_BYTES:
        return shape[1]
    return 0


def sn_scale_rule(shape):
    """A weight in k_sn_scale_m's launch (csrc/spectral.hip:322-333): path, grid, whether the cap makes the loop go round again, LDS."""
    Cout, Cin, KH, KW, K = sn_dims(shape)
    cl = sn_channels_last(shape)
    if cl:                                                                   # :326-332: one block per output channel
        return dict(path="cl", grid=min(Cout, SN_SCALE_CAP), capped=Cout > SN_SCALE_CAP, lds=KH * KW * (cl + 4) * 4)
    n4 = Cout * K // 4
    return dict(path="plain", grid=min(max(cdiv(n4, 1024), 1), SN_SCALE_CAP), capped=cdiv(n4, 1024) > SN_SCALE_CAP, lds=0)


def rows_dense(st, dims, K):
    """ops._rows_dense (ops.py:960-968; csrc/spectral.hip:369-385): every Cout-row a dense permutation of its K elements."""
    run = 1
    for i in sorted(range(3), key=lambda i: st[1 + i]):
        if dims[i] > 1 and st[1 + i] != run:
            return False
        run *= dims[i]
    return st[0] == K


def cot_strides(shape, cot):
    """Element strides (s0, s1, s2, s3) along (Cout, Cin, KH, KW) of the cotangent as the row hands it over."""
    Cout, Cin, KH, KW, K = sn_dims(shape)
    if cot == "contig":
        return (K, KH * KW, KW, 1)
    if cot == "ohwi":                          # [Cout][KH][KW][Cin]: what the weight-gradient kernels write
        return (K, 1, KW * Cin, Cin)
    if cot == "ohiw":                          # [Cout][KH][Cin][KW]: another dense permutation
        return (K, KW, Cin * KW, 1)
    if cot == "padslice":                      # channels [0, Cin) of a [Cout][KH][KW][Cin padded to 4 + 4] buffer
        Cp = cdiv(Cin, 4) * 4 + 4
        return (KH * KW * Cp, 1, KW * Cp, Cp)
    assert cot == "colmajor" and len(shape) == 2   # a 2-D gradient stored transposed
    return (1, Cout, Cout, Cout)


def cot_goes_through_contiguous(shape, cot):
    """The `.contiguous()` fallback of _SpectralWeight.backward (ops.py:927-933)."""
    Cout, Cin, KH, KW, K = sn_dims(shape)
    return len(shape) != 4 and cot != "contig" or not rows_dense(cot_strides(shape, cot), (Cin, KH, KW), K)


def pool3_out(n):
    return (n - 1) // 2 + 1


def launches(c):
    """[(kernel, items handed to ew_grid)] of the row's elementwise launches, forward and backward."""
    e, need = c["entry"], bool(c["need"])
    if c["family"] == "spectral" or c["refuse"]:
        return []
    if e == "l1_mean":                         # perceptual.hip:284,299
        n = int(np.prod(c["shape"]))
        return [("l1_partial", cdiv(n // 4, 4))] + ([("l1_bwd", n // 4)] if need else [])
    if e == "gan_hinge":                       # perceptual.hip:338 (the forward is one block)
        if not hinge_fused(c) or not need:
            return []
        return [("hinge_bwd", max(int(np.prod(s)) for s, _ in c["maps"]))]
    B, C, H, W = c["shape"]
    q = B * C // 4
    if e in ("maxpool2", "avgpool2"):          # perceptual.hip:234,247,259,270
        out = [(e + "_fwd", q * (H // 2) * (W // 2)), (e + "_bwd", q * H * W)]
    elif e == "upsample2x":                    # norm.hip:729,738
        out = [("upsample2x_fwd", q * 4 * H * W), ("upsample2x_bwd", q * H * W)]
    elif e == "nearest_resize":                # norm.hip:707,719
        out = [("nearest_fwd", q * c["out_size"][0] * c["out_size"][1]), ("nearest_bwd", q * H * W)]
    else:                                      # norm.hip:748,760; pool_fanout with only the full consumer runs no backward kernel
        out = [("avgpool3s2_fwd", q * pool3_out(H) * pool3_out(W))]
        out += [("avgpool3s2_bwd", q * H * W)] if c["mode"] != "full" else []
        return out if need else out[:1]
    return out if need else out[:1]


def describe(c):
    """The kernels and launch rules the row reaches, for the measured table."""
    if c["family"] == "spectral":
        if c["entry"] == SWS:
            return "multi x%d (%d + %d)" % (len(c["members"]), SN_MAXT, len(c["members"]) - SN_MAXT)
        Cout, Cin, KH, KW, K = sn_dims(c["shape"])
        r = sn_scale_rule(c["shape"])
        return "R=%d empty=%d kblocks=%d scale=%s%s cot=%s%s" % (
            sn_R(Cout, K), sn_empty_chunks(Cout, K), cdiv(K, 1024), r["path"], "*cap" if r["capped"] else "", c["cot"],
            "->contiguous" if cot_goes_through_contiguous(c["shape"], c["cot"]) else "")
    if c["entry"] == "gan_hinge" and not hinge_fused(c):
        return "torch fallback"
    head = "hinge_mean " if c["entry"] == "gan_hinge" else ""
    return head + " ".join("%s%s" % (k, "*cap" if ew_capped(n) else "") for k, n in launches(c))


def hinge_fused(c):
    """ops.hinge_mean serves the call (ops.py:1968-1974): 1..4 scales of one-channel maps."""
    return 1 <= len(c["maps"]) <= HINGE_MAX_SCALES and all(s[1] == 1 for s, _ in c["maps"])


# ------------------------------------------------------------------------------------------------- the table
def row(name, family, entry, shape=None, cot="contig", scale=1.0, members=None, nograd=(), skip_bwd=(), fmt="nhwc", kind=None,
        maps=None, gout=1.0, mode=None, out_size=None, data="randn", need=None, refuse=None, refuse_at="fwd", seed=0):
    assert family in ("spectral", "loss", "resample") and cot in COTS
    if need is None:
        need = () if data == "nan" else {"spectral": ("w",), "loss": ("a",) if entry == "l1_mean" else ("x",), "resample": ("x",)}[family]
    c = dict(name=name, family=family, entry=entry, shape=None if shape is None else tuple(shape), cot=cot, scale=scale,
             members=members, nograd=tuple(nograd), skip_bwd=tuple(skip_bwd), fmt=fmt, kind=kind,
             maps=None if maps is None else [(tuple(s), f) for s, f in maps], gout=gout, mode=mode,
             out_size=None if out_size is None else tuple(out_size), data=data, need=tuple(need), refuse=refuse,
             refuse_at=refuse_at, seed=seed)
    return c


SW, SWS, L1, HG = "spectral_weight", "spectral_weights", "l1_mean", "gan_hinge"
M35, M19, M3 = (16, 1, 35, 35), (3, 1, 19, 23), (1, 1, 3, 5)                  # hinge maps; M3 has fewer than 1024 elements
HINGE_SCALES = {1: [M19], 2: [M35, M19], 4: [M35, M19, M3, M19]}


def _hinge_rows():
    out = []
    for kind in (0, 1, 2):
        for n, maps in HINGE_SCALES.items():
            for f in ("pad", "contig"):
                out.append(row("hinge_k%d_s%d_%s" % (kind, n, f), "loss", HG, kind=kind, maps=[(m, f) for m in maps],
                               gout=(3.0, -0.75, 2.5)[kind]))
    return out


def _pool_rows(entry):
    p = entry + "_"
    return [
        row(p + "min_1x4x2x2", "resample", entry, (1, 4, 2, 2)),
        row(p + "odd_2x12x7x9", "resample", entry, (2, 12, 7, 9)),          # the last row and column belong to no window
        row(p + "even_2x12x6x8", "resample", entry, (2, 12, 6, 8)),
        row(p + "negative", "resample", entry, (2, 12, 6, 8), data="neg"),  # a maximum that starts from 0 fails
        row(p + "ties_zeros", "resample", entry, (2, 12, 7, 9), data="ties"),   # the first-index rule
        row(p + "nan", "resample", entry, (2, 12, 6, 8), data="nan"),
        row(p + "stride_1x4x2052x2052", "resample", entry, (1, 4, 2052, 2052)),   # output n4 = 1,052,676: beyond the cap
    ]


SN_MEMBERS = ["sn_64x32x3x3", "sn_128x64x4x4", "sn_64x512x3x3", "sn_33x8x3x3", "sn_20x12x1x1", "sn_16x6x4x4", "sn_48x100",
              "sn_2052x4x3x3", "sn_2056x4096x1x1", "sn_8x960x4x4", "sn_8x1024x4x4", "sn_eps", "sn_1x16x3x3"]

CASES = [
    # ---- spectral normalisation: three training-mode calls, a backward, an eval call, a backward
    row("sn_64x32x3x3", "spectral", SW, (64, 32, 3, 3), cot="ohwi"),                 # channels-last path
    row("sn_128x64x4x4", "spectral", SW, (128, 64, 4, 4)),                           # K = 1024: exactly one column block
    row("sn_64x512x3x3", "spectral", SW, (64, 512, 3, 3), cot="ohiw"),               # K = 4608: 5 column blocks, R capped at 32
    row("sn_1x16x3x3", "spectral", SW, (1, 16, 3, 3), cot="ohwi"),                   # R = 1, a scalar u
    row("sn_33x8x3x3", "spectral", SW, (33, 8, 3, 3), cot="ohiw"),                   # R = 32, per = 2: 15 empty chunks
    row("sn_20x12x1x1", "spectral", SW, (20, 12, 1, 1), cot="ohwi"),                 # 1 x 1: plain layout
    row("sn_16x6x4x4", "spectral", SW, (16, 6, 4, 4), cot="padslice"),               # Cin % 4 != 0: plain layout; .contiguous()
    row("sn_48x100", "spectral", SW, (48, 100)),                                     # a 2-D weight
    row("sn_48x100_colmajor", "spectral", SW, (48, 100), cot="colmajor"),            # its gradient stored transposed
    row("sn_2052x4x3x3", "spectral", SW, (2052, 4, 3, 3), cot="ohwi"),               # channels-last, Cout > 2048: the co loop
    row("sn_2056x4096x1x1", "spectral", SW, (2056, 4096, 1, 1)),                     # plain, n4 = 2,105,344 > 2048 * 1024
    row("sn_8x960x4x4", "spectral", SW, (8, 960, 4, 4), cot="ohwi"),                 # K = 15360; a 61,696-byte transpose buffer
    row("sn_8x1024x4x4", "spectral", SW, (8, 1024, 4, 4), refuse="at most 15360", refuse_at="bwd"),   # forward: plain layout
    row("sn_40x2048x3x3", "spectral", SW, (40, 2048, 3, 3), refuse="at most 15360", refuse_at="bwd"),   # K = 18432: R = 512 // 18
    row("sn_refuse_k27", "spectral", SW, (8, 3, 3, 3), refuse=r"K % 4 == 0"),
    # both norms fall under eps = 1e-12 (||W^T u|| ~ 1e-13, ||W v|| ~ 1e-14) and both clamps act; every quantity stays a
    # normal fp32 number (tests/test_loss_cases.py)
    row("sn_eps", "spectral", SW, (64, 32, 3, 3), cot="ohwi", scale=1e-14),
    # 13 weights: a chunk of 12 whose grid comes from its largest members (every early-return guard is taken), then one alone
    row("sn_multi13", "spectral", SWS, members=SN_MEMBERS, nograd=("sn_20x12x1x1",), skip_bwd=("sn_8x1024x4x4",)),
    # ---- L1
    row("l1_n4", "loss", L1, (1, 4, 1, 1)),
    row("l1_nchw", "loss", L1, (2, 8, 5, 7), fmt="nchw"),
    row("l1_nhwc", "loss", L1, (2, 8, 5, 7)),
    row("l1_zeros", "loss", L1, (2, 8, 5, 7), data="zeros"),                         # sign(0) = 0
    row("l1_stride_4x64x260x260", "loss", L1, (4, 64, 260, 260)),                    # 17.3 M elements: the partial sums loop on
    row("l1_gout", "loss", L1, (2, 8, 5, 7), gout=-2.5),
    row("l1_nan", "loss", L1, (2, 8, 5, 7), data="nan"),
    row("l1_refuse_strides", "loss", L1, (2, 8, 5, 7), fmt="mixed", refuse="share shape and memory layout"),
    row("l1_refuse_not_dense", "loss", L1, (2, 8, 5, 7), fmt="sliced", refuse="must be dense"),
    row("l1_refuse_n6", "loss", L1, (1, 3, 1, 2), fmt="nchw", refuse="not a multiple of 4"),
] + _hinge_rows() + [
    row("hinge_5scales_fallback", "loss", HG, kind=1, maps=[(M19, "pad"), (M3, "contig"), (M19, "contig"), (M3, "pad"), (M19, "pad")],
        gout=1.5),
    row("hinge_2ch_fallback", "loss", HG, kind=2, maps=[((3, 2, 19, 23), "contig"), (M3, "contig")], gout=1.5),
    row("hinge_big_k1", "loss", HG, kind=1, maps=[((1, 1, 1040, 1040), "contig")], gout=2.0),      # 1,081,600: k_hinge_bwd's cap
    row("hinge_nan_k0", "loss", HG, kind=0, maps=[(M35, "pad"), (M19, "pad")], data="nan"),
    row("hinge_nan_k1", "loss", HG, kind=1, maps=[(M35, "pad"), (M19, "pad")], data="nan"),
    row("hinge_nan_k2", "loss", HG, kind=2, maps=[(M35, "pad"), (M19, "contig")], data="nan"),
    row("hinge_tie_k1", "loss", HG, kind=1, maps=[(M35, "pad"), (M19, "contig")], data="tie", gout=3.0),
    row("hinge_tie_k2", "loss", HG, kind=2, maps=[(M19, "pad"), (M3, "contig")], data="tie", gout=-2.0),
    # ---- the 2 x 2 pools
] + _pool_rows("maxpool2") + _pool_rows("avgpool2") + [
    row("maxpool2_refuse_c6", "resample", "maxpool2", (1, 6, 4, 4), refuse="bad shape"),
    row("maxpool2_refuse_h1", "resample", "maxpool2", (1, 4, 1, 4), refuse="bad shape"),
    row("avgpool2_refuse_c6", "resample", "avgpool2", (1, 6, 4, 4), refuse="bad shape"),
    row("avgpool2_refuse_h1", "resample", "avgpool2", (1, 4, 1, 4), refuse="bad shape"),
    # ---- AvgPool2d(3, 2, 1, count_include_pad=False), alone and behind pool_fanout
    row("avgpool3s2_2x36x9x9", "resample", "avgpool3s2", (2, 36, 9, 9)),
    row("avgpool3s2_2x36x8x10", "resample", "avgpool3s2", (2, 36, 8, 10)),
    row("avgpool3s2_1x4x1x1", "resample", "avgpool3s2", (1, 4, 1, 1)),
    row("avgpool3s2_1x4x2x1", "resample", "avgpool3s2", (1, 4, 2, 1)),
    row("avgpool3s2_refuse_c6", "resample", "avgpool3s2", (1, 6, 4, 4), refuse="bad shape"),
    row("fanout_both", "resample", "pool_fanout", (2, 36, 9, 9), mode="both"),
    row("fanout_full", "resample", "pool_fanout", (2, 36, 8, 10), mode="full"),
    row("fanout_pool", "resample", "pool_fanout", (2, 36, 9, 9), mode="pool"),
    row("fanout_stride_1x4x2051x2051", "resample", "pool_fanout", (1, 4, 2051, 2051), mode="both"),   # both kernels capped
    # ---- nearest resampling
    row("upsample2x_2x8x5x7", "resample", "upsample2x", (2, 8, 5, 7)),
    row("upsample2x_stride_1x4x1026x1026", "resample", "upsample2x", (1, 4, 1026, 1026)),   # 16.8 M out; backward n4 = 1,052,676
    row("upsample2x_refuse_c6", "resample", "upsample2x", (1, 6, 4, 4), refuse="bad shape"),
    row("nearest_7_to_5", "resample", "nearest_resize", (2, 8, 7, 7), out_size=(5, 5)),
    row("nearest_9x70_to_5x33", "resample", "nearest_resize", (1, 4, 9, 70), out_size=(5, 33)),
    row("nearest_5_to_13", "resample", "nearest_resize", (2, 8, 5, 5), out_size=(13, 13)),
    # float32(14 / 46) and float32(6 / 74) put one destination index each on the other side of an integer than float64 does
    row("nearest_14x6_to_46x74", "resample", "nearest_resize", (2, 8, 14, 6), out_size=(46, 74)),
    row("nearest_identity", "resample", "nearest_resize", (2, 8, 6, 7), out_size=(6, 7)),
    row("nearest_to_1x1", "resample", "nearest_resize", (2, 8, 7, 9), out_size=(1, 1)),
    row("nearest_from_1x1", "resample", "nearest_resize", (2, 8, 1, 1), out_size=(4, 6)),
    row("nearest_stride_1030_to_1100x1050", "resample", "nearest_resize", (1, 4, 1030, 1030), out_size=(1100, 1050)),
    row("nearest_refuse_c6", "resample", "nearest_resize", (1, 6, 4, 4), out_size=(3, 3), refuse="multiple of 4"),
]
BY_NAME = {c["name"]: c for c in CASES}


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


# ------------------------------------------------------------------------------------------------- data
def _f32(t):
    """Values every precision can hold: the inputs of a row are float32 numbers."""
    return t.to(torch.float32).to(torch.float64)


def _gen(c):
    return torch.Generator().manual_seed((zlib.crc32(c["name"].encode()) + c["seed"]) & 0x7FFFFFFF)


def _unit(t):
    return t / t.norm()


HINGE_CENTRE = {0: 0.0, 1: 1.0, 2: -1.0}          # where the kind's margin vanishes (kind 0 has none)
QUANTUM = 1.0 / 256                                # pool data are multiples of this: winners tie exactly or lead by 3.9e-3


def make_data(c):
    """The row's inputs and incoming gradients: float64 CPU tensors holding float32 values."""
    g = _gen(c)
    rn = lambda *s: _f32(torch.randn(*s, generator=g, dtype=torch.float64))
    if c["family"] == "spectral":
        if c["entry"] == SWS:
            return dict(members=[make_data(BY_NAME[m]) for m in c["members"]])
        Cout, Cin, KH, KW, K = sn_dims(c["shape"])
        return dict(w=_f32(rn(*c["shape"]) * c["scale"]), u=_f32(_unit(rn(Cout))), v=_f32(_unit(rn(K))),
                    cots=[rn(*c["shape"]), rn(*c["shape"])])
    if c["entry"] == L1:
        b = rn(*c["shape"])
        sgn = torch.randint(0, 2, c["shape"], generator=g).to(torch.float64) * 2 - 1
        a = _f32(b + sgn * (0.25 + torch.rand(c["shape"], generator=g, dtype=torch.float64)))     # |a - b| >= 0.25 - rounding
        if c["data"] == "zeros":
            a[:, :, :2] = b[:, :, :2]
        if c["data"] == "nan":
            a[1, 3, 2, 4] = float("nan")
        return dict(a=a, b=b)
    if c["entry"] == HG:
        xs, pads = [], []
        for i, (s, f) in enumerate(c["maps"]):
            sgn = torch.randint(0, 2, s, generator=g).to(torch.float64) * 2 - 1
            x = _f32(HINGE_CENTRE[c["kind"]] + sgn * (0.01 + (1 + i % 2) * rn(*s).abs()))       # |margin| >= 0.01 - rounding
            if c["data"] == "tie":
                x.view(-1)[::3] = HINGE_CENTRE[c["kind"]]
            if c["data"] == "nan" and i == min(1, len(c["maps"]) - 1):
                x.view(-1)[x.numel() // 2] = float("nan")
            xs.append(x)
            pads.append(rn(s[0], 3, s[2], s[3]) if f == "pad" else None)
        return dict(xs=xs, pads=pads)
    B, C, H, W = c["shape"]
    x = torch.round(rn(B, C, H, W) * 256) * QUANTUM
    if c["data"] == "neg":
        x = -(x.abs() + 1.0)
    if c["data"] == "ties":
        x = torch.randint(-1, 2, (B, C, H, W), generator=g).to(torch.float64)                    # -1, 0, 1
    if c["data"] == "nan":
        x[1, 5, 2, 3] = float("nan")               # one window of one channel
    e = c["entry"]
    if e in ("maxpool2", "avgpool2"):
        out = [(B, C, H // 2, W // 2)]
    elif e == "upsample2x":
        out = [(B, C, 2 * H, 2 * W)]
    elif e == "nearest_resize":
        out = [(B, C) + c["out_size"]]
    elif e == "avgpool3s2":
        out = [(B, C, pool3_out(H), pool3_out(W))]
    else:
        out = [(B, C, H, W), (B, C, pool3_out(H), pool3_out(W))]
    return dict(x=x, douts=[rn(*s) for s in out])


# ------------------------------------------------------------------------------------------------- ref64
def _normalize(x, eps):
    return x / x.norm().clamp_min(eps)


def spectral_call(W2, u, v, iterate, eps=SN_EPS):
    """One call of `SpectralNorm.compute_weight` on W2 = W.view(Cout, -1): (u, v, sigma) — one power iteration in training
    mode, none in eval; W_eff = W / sigma."""
    if iterate:
        v = _normalize(W2.t() @ u, eps)
        u = _normalize(W2 @ v, eps)
    return u, v, torch.dot(u, W2 @ v)


def spectral_bwd(G2, W2, u, v, sigma):
    """dW = (dW_eff - (sum dW_eff . W_eff) u v^T) / sigma with u, v constants."""
    return (G2 - (G2 * (W2 / sigma)).sum() * torch.outer(u, v)) / sigma


def _spectral(c, d, dtype, need_w=True, skip_bwd=False):
    """Three training-mode calls, the backward of call 3, an eval call, its backward."""
    W = d["w"].to(dtype)
    W2, u, v = W.reshape(W.shape[0], -1), d["u"].to(dtype), d["v"].to(dtype)
    res = {}
    for k in (1, 2, 3):
        u, v, sigma = spectral_call(W2, u, v, True)
        res.update({"weff%d" % k: W / sigma, "u%d" % k: u, "v%d" % k: v, "sigma%d" % k: sigma.reshape(1)})
    back = need_w and not skip_bwd and not c["refuse"]
    res["dw3"] = spectral_bwd(d["cots"][0].to(dtype).reshape(W2.shape), W2, u, v, sigma).reshape(W.shape) if back else None
    u, v, sigma = spectral_call(W2, u, v, False)
    res.update(weff_e=W / sigma, sigma_e=sigma.reshape(1))
    res["dw_e"] = spectral_bwd(d["cots"][1].to(dtype).reshape(W2.shape), W2, u, v, sigma).reshape(W.shape) if back else None
    return res


def _hinge(c, d, dtype):
    """(1/n) sum_i -mean(term(x_i)), term = x | min(x - 1, 0) | min(-x - 1, 0) (oracle/functional.py:463-475); on the
    margin the gradient takes torch.min's 1/2."""
    kind, n = c["kind"], len(c["maps"])
    total, res = 0.0, {}
    for i, x in enumerate(x.to(dtype) for x in d["xs"]):
        m = x if kind == 0 else (x - 1 if kind == 1 else -x - 1)
        term = m if kind == 0 else torch.where(m < 0, m, torch.zeros_like(m)) + (m - m)        # (m - m: a NaN stays one)
        total = total + -(term.sum() / x.numel())
        if c["need"]:
            slope = torch.ones_like(x) if kind == 0 else (m < 0).to(dtype) + 0.5 * (m == 0).to(dtype)
            res["dx%d" % i] = slope * (-1.0 if kind == 2 else 1.0) * (-c["gout"] / (x.numel() * n))
    res["loss"] = (total / n).reshape(1)
    return res


def windows2(x):
    """(B, C, OH, OW, 4): the 2 x 2 windows in row-major order."""
    OH, OW = x.shape[2] // 2, x.shape[3] // 2
    return torch.stack([x[:, :, dy:2 * OH:2, dx:2 * OW:2] for dy in (0, 1) for dx in (0, 1)], -1)


def _maxpool2(x, dout):
    """Forward and the gradient: to the FIRST maximum of the window in row-major order; a NaN wins (the last one if several:
    ATen's `val > max || isnan(val)`)."""
    w = windows2(x)
    nan = torch.isnan(w)
    mx = torch.where(nan.any(-1), torch.full_like(w[..., 0], float("nan")), torch.nan_to_num(w, nan=-float("inf")).max(-1).values)
    hit = torch.where(nan.any(-1, keepdim=True), nan & (nan.flip(-1).cumsum(-1).flip(-1) == 1), w == mx.unsqueeze(-1))
    first = hit & (hit.cumsum(-1) == 1)
    dx = torch.zeros_like(x)
    OH, OW = mx.shape[2], mx.shape[3]
    for k, (dy, dxx) in enumerate((a, b) for a in (0, 1) for b in (0, 1)):
        dx[:, :, dy:2 * OH:2, dxx:2 * OW:2] = first[..., k].to(x.dtype) * dout
    return mx, dx


def nearest_index(n_out, n_in):
    """min(floor(dst * float32(in / out)), in - 1) in float32 arithmetic, as ATen and csrc/norm.hip:409 compute it."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(src, n_in - 1))


def _resample_fn(c, x):
    """The row's outputs as differentiable plain tensor code."""
    e = c["entry"]
    B, C, H, W = x.shape
    if e == "avgpool2":
        return [windows2(x).sum(-1) / 4]
    if e == "upsample2x":
        return [x[:, :, torch.arange(2 * H) // 2][:, :, :, torch.arange(2 * W) // 2]]
    if e == "nearest_resize":
        return [x[:, :, nearest_index(c["out_size"][0], H)][:, :, :, nearest_index(c["out_size"][1], W)]]
    OH, OW = pool3_out(H), pool3_out(W)                       # 3 x 3, stride 2, pad 1, divided by the taps inside the map
    xp = torch.zeros(B, C, 2 * OH + 1, 2 * OW + 1, dtype=x.dtype)
    inside = torch.zeros(1, 1, 2 * OH + 1, 2 * OW + 1, dtype=x.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    inside[:, :, 1:H + 1, 1:W + 1] = 1
    taps = lambda t: sum(t[:, :, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] for ky in range(3) for kx in range(3))
    pooled = taps(xp) / taps(inside)
    return [pooled] if e == "avgpool3s2" else [x * 1, pooled]


def _used(c):
    """Which outputs the row's loss reads."""
    return {"both": (0, 1), "full": (0,), "pool": (1,)}[c["mode"]] if c["entry"] == "pool_fanout" else (0,)


def evaluate(c, d, dtype=torch.float64):
    """{tensor name: tensor or None} of row `c` in `dtype`: float64 is `ref64`; float32 is the same function in the kernels'
    number format, the yardstick of the banded tensors."""
    if c["family"] == "spectral":
        if c["entry"] == SW:
            return _spectral(c, d, dtype)
        res = {}
        for i, (m, dm) in enumerate(zip(c["members"], d["members"])):
            r = _spectral(dict(BY_NAME[m], refuse=None), dm, dtype, m not in c["nograd"], m in c["skip_bwd"])
            res.update({"m%02d.%s" % (i, k): t for k, t in r.items()})
        return res
    if c["entry"] == L1:
        a, b = d["a"].to(dtype), d["b"].to(dtype)
        diff = a - b
        res = dict(loss=diff.abs().sum() / diff.numel())
        if c["need"]:
            res["da"] = torch.sign(diff) * (c["gout"] / diff.numel())
        return res
    if c["entry"] == HG:
        return _hinge(c, d, dtype)
    x = d["x"].to(dtype)
    if c["entry"] == "maxpool2":
        y, dx = _maxpool2(x, d["douts"][0].to(dtype))
        return dict(out0=y, dx=dx if c["need"] else None)
    x = x.clone().requires_grad_(bool(c["need"]))
    outs = _resample_fn(c, x)
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    res["dx"] = None
    if c["need"]:
        sum((outs[i] * d["douts"][i].to(dtype)).sum() for i in _used(c)).backward()
        res["dx"] = x.grad
    return res


def ref64(c, d):
    return evaluate(c, d, torch.float64)


def rule(c, name):
    """What a tensor of the row is held to on the device: "exact" (pure selections and copies), "band" (the spectral
    backward and everything of a weight scaled towards eps: no fixed fraction can be derived), "scalar" (a loss value) or
    "gate"."""
    if c["family"] == "spectral":
        m = BY_NAME[c["members"][int(name[1:3])]] if c["entry"] == SWS else c
        return "band" if name.split(".")[-1].startswith("dw") or m["scale"] != 1.0 else "gate"
    if name == "loss":
        return "scalar"
    if c["entry"] == "maxpool2" or (name == "out0" and c["entry"] in ("upsample2x", "nearest_resize", "pool_fanout")):
        return "exact"
    return "gate"


# ------------------------------------------------------------------------------------------------- discontinuities
def hinge_margins(c, d):
    """Every prediction's margin (kinds 1 and 2), NaNs left out."""
    m = torch.cat([(x - 1 if c["kind"] == 1 else -x - 1).reshape(-1) for x in d["xs"]])
    return m[~torch.isnan(m)]


def maxpool_leads(x):
    """Per window: by how much the winner leads the best value that is not bit-equal to it (inf: all four tie)."""
    w = windows2(torch.nan_to_num(x, nan=float("inf")))
    mx = w.max(-1, keepdim=True).values
    rest = torch.where(w == mx, torch.full_like(w, -float("inf")), w).max(-1).values
    return mx.squeeze(-1) - rest
