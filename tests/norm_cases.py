"""The normalisation / SPADE path matrix: one row per code path (and per kernel corner) that can serve a normalisation
layer, with `norm_ref64`, a plain float64 CPU restatement of the family's contract (reference
sync_batchnorm/batchnorm.py:63-93,128-145, normalization.py:96-110, architecture.py:37-68).  Used by
tests/test_gpu_norm_paths.py (each row through the entry point it names on the device) and tests/test_norm_cases.py (on
the CPU: the reference against torch autograd, the table's coverage, the masking cap).

A row (dict, built by `row`) holds
  name, path      — the id and the autograd Function that must serve it: "_NormAct", "_NormActPair", "_SpadeJoined" or
                    "_SpadeFused"
  via             — how it is called: "ops" (ops.norm_act / norm_act_pair / spade_joined / spade_fused directly),
                    "affine2d" (BatchNormAct), "affine1d" (BatchNorm1dAct), "affine_sync" (an affine
                    SynchronizedBatchNorm2d), "spade" (SPADE.forward), "pair" (spade_pair on a SPADEResnetBlock's norm_s /
                    norm_0) or "block0" (norm_0 of a block without learned shortcut)
  calls           — the ops entry points the row must reach, in order
  B, C, H, W      — the 4-d view of x; `shape`: the shape the module is given ((N, C) / (N, C, L)) if not that
  instance, training, multi — statistics over G = B groups; eval mode; the N-replica form (max(var, eps), run in the child)
  mod             — "none" | "gb" (gamma || beta given) | "conv" (gamma || beta = conv3x3(actv, w) + b) | "affine" | "seg"
                    (through the SPADE module: mlp_shared, then the joined convolution)
  K, slopes       — modulations of the same normalised x and their LeakyReLU slopes
  nh, in_slope    — hidden channels of each modulation's actv; the slope of the ReLU that made actv (None: actv is free)
  running         — per modulation: whether it has running buffers;  momentum, eps
  need            — what requires grad: "x", "g" (gamma || beta map), "a" (actv / seg), "w", "b" (convolution / affine)
  xfmt            — "nchw" | "cl" | "slice" (as conv_cases)
  offset, const, sigma — x = offset + sigma * randn; `const`: that channel is the constant 1.5 (var = 0)
  launch          — _SpadeFused: per modulation "pair" or "joint", what ops.WINO4_AUDIT must show
  knobs, persistent — ops attributes to set; csg_wino4_persistent() off for the row
  mean_term       — the allowance gets the fp32-mean term (see test_gpu_norm_paths.tolerance): offset rows only
  seed            — added to the data generator's seed (crc32 of the name): moved when the fp64 reference alone masks
                    more than MASK_CAP of a row (a row of 576 elements may mask none)
  refuse          — the call must raise a RuntimeError matching this pattern
"""
import zlib

import torch
import torch.nn.functional as F

from conv_cases import LEAKY, NONE, conv2d_ref64, kink_mask

PATHS = ("_NormAct", "_NormActPair", "_SpadeJoined", "_SpadeFused")
ENTRY = {"_NormAct": "norm_act", "_NormActPair": "norm_act_pair", "_SpadeJoined": "spade_joined", "_SpadeFused": "spade_fused"}
MI355X_CUS = 256          # w4_persistent_blocks: one block per CU rounded down to 8; the joint launch needs 2 items per block
SEG_NC, NHIDDEN = 8, 128  # label channels of the module rows; SPADE's hidden width
MASK_CAP = 1e-3           # a row may mask at most 0.1 % of its incoming gradient


def row(name, path, B, C, H, W, instance=False, training=True, multi=False, mod="none", K=1, slopes=(1.0,), nh=None,
        in_slope=0.0, running=None, momentum=0.1, eps=1e-5, need=None, xfmt="nchw", offset=0.3, sigma=1.7, const=None,
        via="ops", shape=None, calls=None, launch=None, knobs=None, persistent=True, mean_term=False, refuse=None, seed=0):
    assert path in PATHS and len(slopes) == K
    if need is None:
        need = {"none": "x", "gb": "xg", "conv": "xawb", "affine": "xwb", "seg": "xawb"}[mod]
    if running is None:
        running = (not instance,) * K
    if nh is None and mod in ("conv", "seg"):
        nh = (NHIDDEN,) * K if mod == "seg" else (32,) * K
    if calls is None:
        calls = [ENTRY[path]]
    return dict(name=name, path=path, B=B, C=C, H=H, W=W, instance=instance, training=training, multi=multi, mod=mod, K=K,
                slopes=tuple(float(s) for s in slopes), nh=nh, in_slope=in_slope, running=tuple(running), momentum=momentum,
                eps=eps, need=need, xfmt=xfmt, offset=offset, sigma=sigma, const=const, via=via, shape=shape, calls=calls,
                launch=launch, knobs=knobs or {}, persistent=persistent, mean_term=mean_term, refuse=refuse, seed=seed)


NA, NP, SJ, SF = PATHS
# a launch the joint form serves on 256 CUs: B * ceil(H / 16) * ceil(W / 32) * C / 32 >= 512 items — partly filled tiles
# (20 x 36: four tiles of 720 pixels) keep the float64 reference of the convolution small
JOINT = dict(B=32, C=128, H=20, W=36)

CASES = [
    # ---- _NormAct: batch / instance x training / eval x {no gamma || beta, gamma || beta} x slope {1, 0.2, 0}
    row("na_batch_plain", NA, 2, 64, 12, 12),
    row("na_batch_plain_lrelu", NA, 3, 8, 5, 7, slopes=(0.2,)),
    row("na_batch_gb", NA, 2, 16, 9, 9, mod="gb"),
    row("na_batch_gb_lrelu", NA, 3, 8, 5, 7, mod="gb", slopes=(0.2,)),
    row("na_batch_gb_relu", NA, 2, 8, 6, 6, mod="gb", slopes=(0.0,), seed=1),
    row("na_inst_plain", NA, 3, 12, 6, 5, instance=True, slopes=(0.2,)),
    row("na_inst_plain_relu", NA, 2, 8, 7, 5, instance=True, slopes=(0.0,)),
    row("na_inst_gb", NA, 2, 8, 6, 6, instance=True, mod="gb", slopes=(0.2,)),
    row("na_inst_eval", NA, 2, 8, 6, 6, instance=True, training=False, slopes=(0.2,)),
    row("na_eval_plain", NA, 2, 8, 6, 6, training=False),
    row("na_eval_gb_lrelu", NA, 2, 8, 6, 6, training=False, mod="gb", slopes=(0.2,)),
    row("na_eval_gb_relu", NA, 2, 8, 6, 6, training=False, mod="gb", slopes=(0.0,)),
    row("na_no_running", NA, 2, 8, 6, 6, mod="gb", slopes=(0.2,), running=(False,), seed=1),
    row("na_momentum", NA, 2, 8, 6, 6, mod="gb", momentum=0.37),
    row("na_x_no_grad", NA, 2, 8, 6, 6, mod="gb", slopes=(0.2,), need="g"),
    row("na_x_cl", NA, 2, 16, 9, 9, mod="gb", slopes=(0.2,), xfmt="cl"),
    row("na_x_slice", NA, 2, 16, 9, 9, mod="gb", slopes=(0.2,), xfmt="slice"),
    # ---- the statistics / reduction kernels' corners
    row("na_c4", NA, 3, 4, 6, 7, mod="gb", slopes=(0.2,)),                    # one quad: 64 row lanes
    row("na_c12", NA, 3, 12, 6, 5, mod="gb", slopes=(0.2,)),                  # 3 quads: 85 row lanes, one thread idle
    row("na_c20", NA, 2, 20, 9, 7, mod="gb", slopes=(0.2,)),                  # 5 quads: 51 row lanes, one thread idle
    row("na_c1024", NA, 2, 1024, 4, 4, mod="gb", slopes=(0.2,)),              # 256 quads: one row lane, P = 32
    row("na_c1040", NA, 2, 1040, 9, 9, mod="gb", slopes=(0.2,)),              # second qb pass of 4 quads, 5 chunks
    row("na_c2048", NA, 2, 2048, 4, 4, mod="gb", slopes=(0.2,)),              # two full qb passes
    row("na_c2048_inst", NA, 2, 2048, 6, 6, instance=True, slopes=(0.2,)),
    row("na_p_small", NA, 1, 8, 3, 5, mod="gb", slopes=(0.2,)),               # P = 15 < 32: one chunk
    row("na_p40000", NA, 4, 8, 100, 100, mod="gb", slopes=(0.2,)),            # per = 40: 24 empty trailing chunks
    row("na_p40000_plain", NA, 1, 8, 200, 200),
    row("na_inst_129", NA, 2, 8, 129, 129, instance=True, slopes=(0.2,)),     # the PatchGAN's plane
    row("na_40x40_c128", NA, 4, 128, 40, 40, mod="gb", slopes=(0.2,)),
    row("na_inst_33", NA, 2, 8, 33, 33, instance=True, slopes=(0.2,)),
    # ---- offset inputs (mean / sigma = 100) and zero variance
    row("na_offset_batch", NA, 2, 16, 24, 24, mod="gb", slopes=(0.2,), offset=170.0, mean_term=True),
    row("na_offset_inst_129", NA, 2, 8, 129, 129, instance=True, slopes=(0.2,), offset=170.0, mean_term=True),
    row("na_const_channel", NA, 2, 8, 6, 6, mod="gb", slopes=(0.2,), const=5),
    # ---- affine norms through the modules (gamma || beta is the broadcast weight - 1 || bias)
    row("affine2d_n3", NA, 3, 8, 5, 6, mod="affine", slopes=(0.2,), via="affine2d"),
    row("affine2d_n1", NA, 1, 8, 4, 4, mod="affine", slopes=(0.2,), via="affine2d"),
    row("affine2d_eval", NA, 3, 8, 5, 6, mod="affine", slopes=(0.2,), via="affine2d", training=False),
    row("affine1d_nc", NA, 3, 12, 1, 1, mod="affine", slopes=(0.0,), via="affine1d", shape=(3, 12)),
    row("affine1d_nc_count1", NA, 1, 8, 1, 1, mod="affine", slopes=(0.0,), via="affine1d", shape=(1, 8)),
    row("affine1d_ncl", NA, 3, 8, 7, 1, mod="affine", slopes=(0.0,), via="affine1d", shape=(3, 8, 7)),
    row("affine1d_ncl_n1", NA, 1, 8, 7, 1, mod="affine", via="affine1d", shape=(1, 8, 7)),
    row("affine_sync_n3", NA, 3, 8, 4, 5, mod="affine", slopes=(0.2,), via="affine_sync"),
    row("affine_sync_n1", NA, 1, 8, 4, 4, mod="affine", via="affine_sync"),
    # ---- _NormActPair
    row("pair_slopes", NP, 2, 16, 8, 8, mod="gb", K=2, slopes=(1.0, 0.2)),
    row("pair_one_running", NP, 2, 12, 6, 5, mod="gb", K=2, slopes=(0.2, 0.0), running=(False, True)),
    row("pair_c1040", NP, 2, 1040, 4, 4, mod="gb", K=2, slopes=(1.0, 0.2)),
    row("pair_x_no_grad", NP, 2, 16, 8, 8, mod="gb", K=2, slopes=(1.0, 0.2), need="g"),
    # ---- _SpadeJoined: maps below 32 wide
    row("sj_8x8_c64", SJ, 2, 64, 8, 8, mod="conv", slopes=(0.2,)),
    row("sj_16x16_c12", SJ, 2, 12, 16, 16, mod="conv", slopes=(0.2,), in_slope=None),
    row("sj_8x8_c1024", SJ, 2, 1024, 8, 8, mod="conv", slopes=(0.2,), nh=(16,)),
    row("sj_16x16_c20_plain", SJ, 2, 20, 16, 16, mod="conv", slopes=(1.0,)),
    row("sj_need_x_only", SJ, 2, 64, 8, 8, mod="conv", slopes=(0.2,), need="x"),
    row("sj_need_w_only", SJ, 2, 64, 8, 8, mod="conv", slopes=(0.2,), need="w", in_slope=None),
    # ---- _SpadeFused: the launch pair (launches too small for the persistent form)
    row("sf_pair_k1", SF, 2, 64, 32, 32, mod="conv", slopes=(0.2,), launch=("pair",)),
    row("sf_pair_k1_16x32_c32", SF, 2, 32, 16, 32, mod="conv", slopes=(0.2,), launch=("pair",)),
    row("sf_pair_k2_c96", SF, 2, 96, 20, 36, mod="conv", K=2, slopes=(1.0, 0.2), launch=("pair", "pair")),
    row("sf_pair_relu", SF, 2, 32, 16, 32, mod="conv", slopes=(0.0,), launch=("pair",)),
    row("sf_pair_x_no_grad", SF, 2, 32, 16, 32, mod="conv", slopes=(0.2,), need="awb", launch=("pair",)),
    row("sf_pair_w_no_grad", SF, 2, 32, 16, 32, mod="conv", K=2, slopes=(1.0, 0.2), need="xa", launch=("pair", "pair")),
    # ---- _SpadeFused: the joint launch, and what switches it back to the pair
    row("sf_joint_k1", SF, mod="conv", slopes=(0.2,), launch=("joint",), **JOINT),
    row("sf_joint_k2_c96", SF, 44, 96, 20, 36, mod="conv", K=2, slopes=(1.0, 0.2), launch=("joint", "joint")),
    row("sf_joint_relu_in_free", SF, mod="conv", slopes=(0.0,), in_slope=None, need="xa", launch=("joint",), **JOINT),
    row("sf_joint_knob_off", SF, mod="conv", slopes=(0.2,), need="x", launch=("pair",), knobs={"SPADE_JOINT": False}, **JOINT),
    row("sf_joint_persistent_off", SF, mod="conv", slopes=(0.2,), need="x", launch=("pair",), persistent=False, **JOINT),
    # 15 stages -> pair, 16 -> joint: different slopes and weights per modulation, so swapped outputs or gradients fail
    row("sf_mixed_k2", SF, mod="conv", K=2, slopes=(1.0, 0.2), nh=(120, 128), launch=("pair", "joint"), **JOINT),
    row("sf_mixed_k2_rev", SF, mod="conv", K=2, slopes=(0.2, 1.0), nh=(128, 120), need="xw", launch=("joint", "pair"),
        **JOINT),
    # ---- calls the contract refuses
    row("refuse_fused_c48", SF, 2, 48, 16, 32, mod="conv", slopes=(0.2,), refuse="multiple of 32"),
    row("refuse_fused_actv_shape", SF, 2, 32, 16, 32, mod="conv", slopes=(0.2,), refuse="do not fit"),
    row("refuse_affine_with_gb", NA, 3, 8, 4, 5, mod="affine", via="affine_sync", refuse="cannot take a SPADE modulation"),
    # ---- the dispatch: SPADE.forward / spade_pair at sizes that land on each path, training and eval
    row("mod_spade_fused", SF, 2, 64, 16, 32, mod="seg", slopes=(0.2,), via="spade", launch=("pair",)),
    row("mod_spade_joined", SJ, 2, 64, 8, 8, mod="seg", slopes=(0.2,), via="spade"),
    row("mod_spade_eval", NA, 2, 64, 8, 8, mod="seg", slopes=(0.2,), via="spade", training=False),
    row("mod_spade_eval_32", NA, 2, 32, 16, 32, mod="seg", slopes=(1.0,), via="spade", training=False),
    row("mod_spade_instance", NA, 2, 16, 8, 8, mod="seg", slopes=(0.2,), via="spade", instance=True),
    row("mod_block0_joined", SJ, 2, 32, 16, 16, mod="seg", slopes=(0.2,), via="block0"),
    row("mod_block0_fused", SF, 2, 32, 16, 32, mod="seg", slopes=(0.2,), via="block0", launch=("pair",)),
    row("mod_pair_fused", SF, 2, 64, 16, 32, mod="seg", K=2, slopes=(1.0, 0.2), via="pair", launch=("pair", "pair")),
    row("mod_pair_small", NP, 2, 64, 8, 8, mod="seg", K=2, slopes=(1.0, 0.2), via="pair"),
    row("mod_pair_eval", NA, 2, 64, 8, 8, mod="seg", K=2, slopes=(1.0, 0.2), via="pair", training=False,
        calls=["norm_act", "norm_act"]),
    # ---- the N-replica form (one-rank group in a child process): max(var, eps)^-1/2, asynchronous all-reduces
    row("multi_na", NA, 2, 12, 6, 5, multi=True, mod="gb", slopes=(0.2,)),
    row("multi_na_var_below_eps", NA, 2, 8, 6, 6, multi=True, mod="gb", slopes=(0.2,), offset=0.0, sigma=0.003),
    row("multi_na_const_channel", NA, 2, 8, 6, 6, multi=True, mod="gb", slopes=(0.2,), const=2),
    row("multi_pair", NP, 2, 16, 8, 8, multi=True, mod="gb", K=2, slopes=(1.0, 0.2)),
    row("multi_pair_var_below_eps", NP, 2, 8, 6, 6, multi=True, mod="gb", K=2, slopes=(1.0, 0.2), offset=0.0, sigma=0.003),
    row("multi_sj", SJ, 2, 64, 8, 8, multi=True, mod="conv", slopes=(0.2,)),
    row("multi_sj_var_below_eps", SJ, 2, 16, 8, 8, multi=True, mod="conv", slopes=(0.2,), offset=0.0, sigma=0.003),
    row("multi_sf_k1", SF, multi=True, mod="conv", slopes=(0.2,), launch=("pair",), **JOINT),
    row("multi_sf_k2", SF, multi=True, mod="conv", K=2, slopes=(1.0, 0.2), launch=("pair", "pair"), **JOINT),
    row("multi_sf_var_below_eps", SF, 2, 32, 16, 32, multi=True, mod="conv", slopes=(0.2,), launch=("pair",), offset=0.0,
        sigma=0.003),
]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


def joint_items(c):
    """Work items of the row's joint launch: B * tiles (16 rows x 32 columns of the map) * C / 32."""
    return c["B"] * -(-c["H"] // 16) * -(-c["W"] // 32) * (c["C"] // 32)


def joint_rule(c, k):
    """What `w4_persistent_blocks` decides for modulation k of a _SpadeFused row on an MI355X: "joint" with >= 2 items per
    CU (CU count rounded down to 8) and an even number of >= 4 stages (nh / 8), else "pair" — also under N > 1 ranks,
    SPADE_JOINT = False or with the persistent form off."""
    stages = c["nh"][k] // 8
    ok = (not c["multi"] and c["knobs"].get("SPADE_JOINT", True) and c["persistent"] and stages >= 4 and stages % 2 == 0
          and joint_items(c) >= 2 * (MI355X_CUS & ~7))
    return "joint" if ok else "pair"


def shrunk(c):
    """A twin of row `c` small enough for the CPU tests: the same options on a smaller map, batch and hidden width."""
    t = dict(c)
    if c["B"] * c["C"] * c["H"] * c["W"] > 300000:
        if c["mod"] in ("conv", "seg"):
            t.update(B=2, H=min(c["H"], 8), W=min(c["W"], 12), nh=tuple(min(n, 16) for n in c["nh"]))
        else:
            t.update(H=min(c["H"], 24), W=min(c["W"], 24))
    if c["C"] > 256:
        t.update(C=c["C"] // 16 // 4 * 4)
    if c["mod"] in ("conv", "seg") and c["C"] >= 64:
        t.update(C=min(t["C"], 32))
    return t


# ------------------------------------------------------------------------------------ data
def make_data(c):
    """fp32 CPU operands of row `c`: x, dy[k], and per modulation k gb / (actv, w, b) / seg + (w_sh, b_sh, w, b), the
    affine weight and bias, running buffers rm[k], rv[k]."""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()) + c["seed"])
    B, C, H, W, K = c["B"], c["C"], c["H"], c["W"], c["K"]
    x = c["offset"] + c["sigma"] * torch.randn(B, C, H, W, generator=g)
    if c["const"] is not None:
        x[:, c["const"]] = 1.5
    d = dict(x=x, mods=[], dy=[torch.randn(B, C, H, W, generator=g) for _ in range(K)])
    if c["mod"] == "seg":
        d["seg"] = torch.randn(B, SEG_NC, H, W, generator=g)
    if c["mod"] == "affine":
        d["weight"] = 1.0 + 0.5 * torch.randn(C, generator=g)
        d["bias"] = 0.5 * torch.randn(C, generator=g)
    for k in range(K):
        m = dict(rm=0.1 * torch.randn(C, generator=g), rv=0.5 + torch.rand(C, generator=g))
        if c["mod"] == "gb":
            m["gb"] = 0.5 * torch.randn(B, 2 * C, H, W, generator=g)
        elif c["mod"] in ("conv", "seg"):
            nh = c["nh"][k]
            if c["mod"] == "conv":
                a = torch.randn(B, nh, H, W, generator=g)
                if c["in_slope"] is not None:                 # a (Leaky)ReLU output, with exact zeros
                    a = F.leaky_relu(a, c["in_slope"])
                    a[:, :, ::3, ::5] = 0.0
                m["actv"] = a
            else:
                m["w_sh"] = torch.randn(nh, SEG_NC, 3, 3, generator=g) / (9 * SEG_NC) ** 0.5
                m["b_sh"] = 0.5 * torch.randn(nh, generator=g)
            m["w"] = 0.5 * torch.randn(2 * C, nh, 3, 3, generator=g) / (9 * nh) ** 0.5 * (2.0 if c["mod"] == "seg" else 1.0)
            m["b"] = 0.3 * torch.randn(2 * C, generator=g)
        d["mods"].append(m)
    return d


# ------------------------------------------------------------------------------------ the fp64 reference
def _leaky64(pre, slope):
    if slope == 1.0:
        return pre, torch.ones_like(pre)
    return torch.where(pre > 0, pre, pre * slope), torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))


def norm_ref64(x, mods, instance=False, training=True, multi=False, eps=1e-5, momentum=0.1, dys=None, need_x=True,
               gate_actv=None):
    """The contract of the normalisation family in float64 on the CPU, forward and backward written out (no autograd).

    x (B, C, H, W); statistics over G = 1 (batch) or G = B (instance) groups: mean, biased var, invstd = (var + eps)^-1/2,
    or max(var, eps)^-1/2 for the N-replica form (`multi`); eval mode (`training` False, batch) takes mods[0]'s running
    statistics as constants.  `mods`: K dicts with `slope` and one of
        gb                          gamma || beta (B, 2C, H, W) given            (need: "g")
        actv, w, b, in_slope        gamma || beta = conv3x3(actv, w) + b; actv is a LeakyReLU(in_slope) output whose
                                    gradient comes back times its gate (in_slope None: plain)    (need: "a", "w", "b")
        seg, w_sh, b_sh, w, b       actv = relu(conv3x3(seg, w_sh) + b_sh) first (the SPADE module's mlp_shared)
        (none of them)              y = leaky(xhat)
    and optionally rm, rv: running buffers, updated in training batch mode with the unbiased variance (count 1: the
    biased one) and `momentum`.  y_k = leaky(xhat (1 + gamma_k) + beta_k, slope_k).
    With `dys` the gradients of sum_k sum(y_k dy_k): dx (over all modulations; eval: no statistics term; N-replica form:
    no invstd term where var < eps, where the clamp is flat), and per modulation dgb or dactv / dw / db (and dseg / dw_sh /
    db_sh).  Only what `need_x` / each mod's `need` asks for is returned, the rest is None.
    `gate_actv`: per modulation, the tensor whose sign the inner ReLU's gate reads if not the fp64 actv."""
    x = x.double()
    if not (training or instance) and len(mods) > 1:      # eval: every modulation has its own statistics — K single calls
        parts = [norm_ref64(x, [m], instance, training, multi, eps, momentum, None if dys is None else [dys[k]], need_x,
                            None if gate_actv is None else [gate_actv[k]]) for k, m in enumerate(mods)]
        out = dict(parts[0], y=[p["y"][0] for p in parts], pre=[p["pre"][0] for p in parts],
                   mods=[p["mods"][0] for p in parts])
        if dys is not None and need_x:
            out["dx"] = sum(p["dx"] for p in parts)
        return out
    B, C, H, W = x.shape
    dims = (2, 3) if instance else (0, 2, 3)
    n = H * W if instance else B * H * W
    if training or instance:
        mean = x.mean(dims, keepdim=True)
        var = ((x - mean) ** 2).mean(dims, keepdim=True)
        live = torch.ones_like(var)
        if multi:
            invstd = var.clamp(min=eps) ** -0.5
            live = (var >= eps).double()
        else:
            invstd = (var + eps) ** -0.5
    else:
        mean = mods[0]["rm"].double().view(1, C, 1, 1)
        var = mods[0]["rv"].double().view(1, C, 1, 1)
        invstd = (var + eps) ** -0.5
    xhat = (x - mean) * invstd
    out = dict(mean=mean, var=var, invstd=invstd, xhat=xhat, y=[], pre=[], dx=None, mods=[])
    gbs, inner = [], []
    for k, m in enumerate(mods):
        r = dict(dgb=None, dactv=None, dw=None, db=None, dseg=None, dw_sh=None, db_sh=None, rm=None, rv=None)
        if m.get("rm") is not None:
            rm, rv = m["rm"].double(), m["rv"].double()
            if training and not instance:
                unb = var * n / (n - 1) if n > 1 else var
                rm = (1 - momentum) * rm + momentum * mean.flatten()
                rv = (1 - momentum) * rv + momentum * unb.flatten()
            r["rm"], r["rv"] = rm, rv
        actv = None
        if m.get("seg") is not None:
            sh = conv2d_ref64(m["seg"], m["w_sh"], m["b_sh"], 1, 1, LEAKY, 0.0)
            actv = sh["y"]
            r["pre_sh"], r["actv"] = sh["pre"], actv
        elif m.get("actv") is not None:
            actv = m["actv"].double()
        if actv is not None:
            gb = conv2d_ref64(actv, m["w"], m["b"], 1, 1)["y"]
        else:
            gb = m["gb"].double() if m.get("gb") is not None else None
        pre = xhat * (1 + gb[:, :C]) + gb[:, C:] if gb is not None else xhat
        y, gate = _leaky64(pre, float(m["slope"]))
        out["y"].append(y)
        out["pre"].append(pre)
        out["mods"].append(r)
        gbs.append(gb)
        inner.append(actv)
    if dys is None:
        return out
    dn = torch.zeros_like(x)
    for k, m in enumerate(mods):
        r, gb, need = out["mods"][k], gbs[k], m.get("need", "")
        dpre = dys[k].double() * _leaky64(out["pre"][k], float(m["slope"]))[1]
        if gb is None:
            dn = dn + dpre
            continue
        dn = dn + dpre * (1 + gb[:, :C])
        dgb = torch.cat([dpre * xhat, dpre], 1)
        if inner[k] is None:
            r["dgb"] = dgb if "g" in need else None
            continue
        in_slope = 0.0 if m.get("seg") is not None else m.get("in_slope")
        ga = None if gate_actv is None else gate_actv[k]
        cneed = ("x" if "a" in need else "") + "".join(t for t in "wb" if t in need)
        cb = conv2d_ref64(inner[k], m["w"], m["b"], 1, 1, in_act=in_slope, dy=dgb, need=cneed, gate_x=ga)
        r["dw"], r["db"] = cb["dw"], cb["db"]
        if m.get("seg") is None:
            r["dactv"] = cb["dx"]
        elif cb["dx"] is not None:                      # cb["dx"] is the gradient of mlp_shared's pre-activation
            sb = conv2d_ref64(m["seg"], m["w_sh"], m["b_sh"], 1, 1, dy=cb["dx"], need="xwb")
            r["dseg"], r["dw_sh"], r["db_sh"] = sb["dx"], sb["dw"], sb["db"]
    out["dn"] = dn
    out["gam1"] = [None if gb is None else 1 + gb[:, :C] for gb in gbs]
    if need_x:
        if training or instance:
            out["dx"] = invstd * (dn - dn.mean(dims, keepdim=True) - xhat * (dn * xhat).mean(dims, keepdim=True) * live)
        else:
            out["dx"] = invstd * dn
    return out


def ref_mods(c, d):
    """The `mods` argument of norm_ref64 for row `c` on data `d`."""
    mods = []
    for k in range(c["K"]):
        m, dm = dict(slope=c["slopes"][k], need=c["need"]), d["mods"][k]
        if c["running"][k]:
            m.update(rm=dm["rm"], rv=dm["rv"])
        if c["mod"] == "gb":
            m["gb"] = dm["gb"]
        elif c["mod"] == "affine":
            B, C, H, W = d["x"].shape
            m["gb"] = torch.cat([d["weight"].double() - 1.0, d["bias"].double()]).view(1, 2 * C, 1, 1).expand(B, 2 * C, H, W)
            m["need"] = "g"
        elif c["mod"] == "conv":
            m.update(actv=dm["actv"], w=dm["w"], b=dm["b"], in_slope=c["in_slope"])
        elif c["mod"] == "seg":
            m.update(seg=d["seg"], w_sh=dm["w_sh"], b_sh=dm["b_sh"], w=dm["w"], b=dm["b"])
        mods.append(m)
    return mods


def mask_kinks(c, d):
    """Zero the incoming gradients d["dy"][k] where modulation k's fp64 pre-activation lies within rounding of its
    LeakyReLU kink (either side is right there); returns the largest masked fraction over the modulations."""
    fwd = norm_ref64(d["x"], ref_mods(c, d), c["instance"], c["training"], c["multi"], c["eps"], c["momentum"])
    worst = 0.0
    for k in range(c["K"]):
        if c["slopes"][k] != 1.0:
            keep = kink_mask(fwd["pre"][k])
            d["dy"][k] = (d["dy"][k].double() * keep).float()
            worst = max(worst, 1.0 - float(keep.mean()))
    return worst


def flatten(c, r):
    """{tensor name: fp64 expectation or None} of row `c` from norm_ref64's result `r`, under the names the device run
    uses: y0, y1, dx, per modulation dgb / dactv / dw / db / dw_sh / db_sh / rm / rv, the summed dseg, the affine dweight
    and dbias."""
    out = {"dx": r["dx"]}
    C = c["C"]
    for k in range(c["K"]):
        out["y%d" % k] = r["y"][k]
        m = r["mods"][k]
        if c["running"][k] and not c["instance"]:
            out["rm%d" % k], out["rv%d" % k] = m["rm"], m["rv"]
        if c["mod"] == "gb":
            out["dgb%d" % k] = m["dgb"]
        elif c["mod"] == "affine":
            dgb = m["dgb"].sum((0, 2, 3))
            out["dweight"] = dgb[:C] if "w" in c["need"] else None
            out["dbias"] = dgb[C:] if "b" in c["need"] else None
        elif c["mod"] == "conv":
            out["dactv%d" % k], out["dw%d" % k], out["db%d" % k] = m["dactv"], m["dw"], m["db"]
        elif c["mod"] == "seg":
            out["dw%d" % k], out["db%d" % k] = m["dw"], m["db"]
            out["dw_sh%d" % k], out["db_sh%d" % k] = m["dw_sh"], m["db_sh"]
            if m["dseg"] is not None:
                out["dseg"] = m["dseg"] if out.get("dseg") is None else out["dseg"] + m["dseg"]
            else:
                out.setdefault("dseg", None)
    if c["mod"] == "affine" and c["shape"] is not None:           # what the module hands back for (N, C) / (N, C, L)
        for t in ("dx", "y0"):
            out[t] = None if out[t] is None else out[t].reshape(c["shape"])
    return out


def reference(c, d, gate_actv=None):
    """(flattened fp64 expectations, norm_ref64's full result) of row `c` on data `d` — after mask_kinks(c, d)."""
    r = norm_ref64(d["x"], ref_mods(c, d), c["instance"], c["training"], c["multi"], c["eps"], c["momentum"], d["dy"],
                   "x" in c["need"], gate_actv)
    return flatten(c, r), r


# ------------------------------------------------------------------------------------ the same row in torch autograd
def torch_twin(c, d, dtype):
    """Row `c` on data `d` with torch's own operators and autograd in `dtype` on the CPU (F.batch_norm / F.instance_norm
    where they state the row; sums and a clamp for the N-replica form and for a count of 1, which F.batch_norm refuses):
    float64 checks norm_ref64, float32 measures what fp32 arithmetic of the same row is off by.  Same names as `flatten`."""
    cast = lambda t: t.to(dtype)
    C, K = c["C"], c["K"]
    x = cast(d["x"]).requires_grad_("x" in c["need"])
    leaves, ys, out = {}, [], {}
    n = (c["H"] * c["W"]) if c["instance"] else c["B"] * c["H"] * c["W"]
    rms = [(cast(d["mods"][k]["rm"]).clone(), cast(d["mods"][k]["rv"]).clone()) if c["running"][k] else (None, None)
           for k in range(K)]
    xhats = None
    if c["instance"]:
        xhat = F.instance_norm(x, eps=c["eps"])
    elif not c["training"]:                              # every module normalises with its own running statistics
        xhats = [F.batch_norm(x, rm, rv, None, None, False, c["momentum"], c["eps"]) for rm, rv in rms]
    elif c["multi"] or n == 1:
        mean = x.mean((0, 2, 3), keepdim=True)
        var = ((x - mean) ** 2).mean((0, 2, 3), keepdim=True)
        xhat = (x - mean) * (var.clamp(min=c["eps"]) ** -0.5 if c["multi"] else (var + c["eps"]) ** -0.5)
        unb = var * n / (n - 1) if n > 1 else var
        for rm, rv in rms:
            if rm is not None:
                rm.mul_(1 - c["momentum"]).add_(c["momentum"] * mean.detach().flatten())
                rv.mul_(1 - c["momentum"]).add_(c["momentum"] * unb.detach().flatten())
    else:
        xhat = F.batch_norm(x, rms[0][0], rms[0][1], None, None, True, c["momentum"], c["eps"])
        for rm, rv in rms[1:]:
            if rm is not None:
                F.batch_norm(x.detach(), rm, rv, None, None, True, c["momentum"], c["eps"])
    if c["mod"] == "seg":
        leaves["seg"] = cast(d["seg"]).requires_grad_("a" in c["need"])
    if c["mod"] == "affine":
        leaves["weight"] = cast(d["weight"]).requires_grad_("w" in c["need"])
        leaves["bias"] = cast(d["bias"]).requires_grad_("b" in c["need"])
    for k in range(K):
        dm, gb = d["mods"][k], None
        if xhats is not None:
            xhat = xhats[k]
        if c["mod"] == "gb":
            gb = leaves["gb%d" % k] = cast(dm["gb"]).requires_grad_("g" in c["need"])
        elif c["mod"] == "affine":
            gb = torch.cat([leaves["weight"] - 1.0, leaves["bias"]]).view(1, 2 * C, 1, 1)
        elif c["mod"] in ("conv", "seg"):
            w = leaves["w%d" % k] = cast(dm["w"]).requires_grad_("w" in c["need"])
            b = leaves["b%d" % k] = cast(dm["b"]).requires_grad_("b" in c["need"])
            if c["mod"] == "conv":
                actv = leaves["actv%d" % k] = cast(dm["actv"]).requires_grad_("a" in c["need"])
            else:
                w_sh = leaves["w_sh%d" % k] = cast(dm["w_sh"]).requires_grad_("w" in c["need"])
                b_sh = leaves["b_sh%d" % k] = cast(dm["b_sh"]).requires_grad_("b" in c["need"])
                actv = F.relu(F.conv2d(leaves["seg"], w_sh, b_sh, padding=1))
            gb = F.conv2d(actv, w, b, padding=1)
        pre = xhat * (1 + gb[:, :C]) + gb[:, C:] if gb is not None else xhat
        ys.append(pre if c["slopes"][k] == 1.0 else F.leaky_relu(pre, c["slopes"][k]))
    loss = sum((y * cast(d["dy"][k])).sum() for k, y in enumerate(ys))
    if loss.requires_grad:
        loss.backward()
    grad = lambda t: None if t not in leaves or leaves[t].grad is None else leaves[t].grad
    out["dx"] = x.grad
    for k in range(K):
        out["y%d" % k] = ys[k].detach()
        if c["running"][k] and not c["instance"]:
            out["rm%d" % k], out["rv%d" % k] = rms[k]
        if c["mod"] == "gb":
            out["dgb%d" % k] = grad("gb%d" % k)
        elif c["mod"] == "conv":
            out["dactv%d" % k], out["dw%d" % k], out["db%d" % k] = grad("actv%d" % k), grad("w%d" % k), grad("b%d" % k)
            if out["dactv%d" % k] is not None and c["in_slope"] is not None:      # the contract: times the producer's gate
                a = leaves["actv%d" % k].detach()
                out["dactv%d" % k] = out["dactv%d" % k] * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, c["in_slope"]))
        elif c["mod"] == "seg":
            out["dw%d" % k], out["db%d" % k] = grad("w%d" % k), grad("b%d" % k)
            out["dw_sh%d" % k], out["db_sh%d" % k] = grad("w_sh%d" % k), grad("b_sh%d" % k)
    if c["mod"] == "seg":
        out["dseg"] = grad("seg")
    if c["mod"] == "affine":
        out["dweight"], out["dbias"] = grad("weight"), grad("bias")
        if c["shape"] is not None:
            for t in ("dx", "y0"):
                out[t] = None if out[t] is None else out[t].reshape(c["shape"])
    return out
