"""ops.plan_conv — the one place a convolution's kernels are chosen — and the host-only predicates it is built from, on the CPU
(C-ABI queries only, no launch): the plan of every convolution and linear of the default training step at the batch sizes of
configs C3 / C4 / C5, and one row per call option."""
import pytest

LEAKY, NONE, TANH = 1, 0, 2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import ops
    return ops


def _code(p):
    """'fwd[variant] dx[variant] wgrad', '-' for a direction not planned."""
    return " ".join((p.fwd + str(p.fwd_var or ""), (p.dx + str(p.dx_var or "")) if p.dx else "-", p.wgrad or "-"))


def _rows(B, S, T, O):
    """(name, plan_conv keywords) of the step's convolutions and linears at batch B, S layout channels, T triplets and O
    objects per image: the generator and both PatchGAN scales (tools/conv_shapes.py), the object discriminator (crop_size 32,
    d_obj_arch C4-64-2,C4-128-2,C4-256-2, valid padding), the graph encoder (embedding_dim 32, gconv_dim 128, hidden 512)."""
    from tools.conv_shapes import shapes
    out = []
    for name, cin, cout, h, k, s, p, _ in shapes(256, S=S):
        kw = dict(B=B, IH=h, IW=h, Cin=cin, Cout=cout, KH=k, KW=k, stride=s, pad=p, has_bias=not name.endswith("conv_s"))
        if name == "conv_img":
            kw.update(Cout=4, act=TANH, cout_real=3, pre_slope=0.2)
        elif name.endswith("model4"):
            kw.update(Cout=4, cout_real=1)
        elif name.endswith("mlp_shared") or (name.startswith("D") and not name.endswith("model3")):
            kw.update(act=LEAKY)
        elif ".gamma_beta" in name:
            kw.update(in_act=(LEAKY, 0.0))
        out.append((name, kw))
    M = B * O
    for name, cin, cout, h in (("objD.C4-64", 4, 64, 32), ("objD.C4-128", 64, 128, 15), ("objD.C4-256", 128, 256, 6)):
        out.append((name, dict(B=M, IH=h, IW=h, Cin=cin, Cout=cout, KH=4, KW=4, stride=2, pad=0, act=LEAKY, has_bias=True)))
    for name, rows, cin, cout, act in (("objD.fc", O, 256, 1024, NONE), ("objD.obj_classifier", O, 1024, 184, NONE),
                                        ("objD.real_classifier", O, 1024, 4, NONE),
                                        ("gconv0.net1.0", T, 160, 512, LEAKY), ("gconv.net1.0", T, 384, 512, LEAKY),
                                        ("gconv.net1.2", T, 512, 1152, LEAKY), ("gconv.net2.0", O, 512, 512, LEAKY),
                                        ("gconv.net2.2", O, 512, 128, LEAKY), ("box_net.0", O, 128, 512, LEAKY),
                                        ("box_net.2", O, 512, 4, NONE)):
        kw = dict(B=B * rows, IH=1, IW=1, Cin=cin, Cout=cout, KH=1, KW=1, stride=1, pad=0, act=act, has_bias=True)
        if name == "objD.real_classifier":
            kw.update(cout_real=1)
        elif name.endswith(".2"):
            kw.update(in_act=(LEAKY, 0.0))
        out.append((name, kw))
    return out


# the parent commit's per-direction choices, differentiated in all three operands: (C3 batch 16, C4 batch 4, C5 batch 6 with
# 128 layout channels and dense graphs)
STEP_PLANS = {
    "fc":                          ("wino2 wino2 wino", "direct direct direct", "direct direct direct"),
    "head_0.mlp_shared":           ("wino2 wino2 wino", "direct direct direct", "direct direct direct"),
    "head_0.gamma_beta[1024]":     ("wino2 wino2 wino4w", "direct direct direct", "direct direct direct"),
    "head_0.conv_0":               ("wino2 wino2 wino4w", "direct direct direct", "direct direct direct"),
    "head_0.conv_1":               ("wino2 wino2 wino4w", "direct direct direct", "direct direct direct"),
    "G_middle_0.mlp_shared":       ("wino2 wino2 wino", "wino2 wino2 wino", "wino2 wino2 wino4w"),
    "G_middle_0.gamma_beta[1024]": ("wino2 wino2 wino4w", "wino2 wino2 wino4w", "wino2 wino2 wino4w"),
    "G_middle_0.conv_0":           ("wino2 wino2 wino4w", "wino2 wino2 wino4w", "wino2 wino2 wino4w"),
    "G_middle_0.conv_1":           ("wino2 wino2 wino4w", "wino2 wino2 wino4w", "wino2 wino2 wino4w"),
    "G_middle_1.mlp_shared":       ("wino2 wino2 wino", "wino2 wino2 wino", "wino2 wino2 wino4w"),
    "G_middle_1.gamma_beta[1024]": ("wino2 wino2 wino4w", "wino2 wino2 wino4w", "wino2 wino2 wino4w"),
    "G_middle_1.conv_0":           ("wino2 wino2 wino4w", "wino2 wino2 wino4w", "wino2 wino2 wino4w"),
    "G_middle_1.conv_1":           ("wino2 wino2 wino4w", "wino2 wino2 wino4w", "wino2 wino2 wino4w"),
    "up_0.mlp_shared":             ("wino2 wino2 wino", "wino2 wino2 wino", "wino2 wino2 wino4w"),
    "up_0.gamma_beta[512]":        ("wino4 wino4 wino4w", "wino2 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_0.gamma_beta[1024]":       ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_0.conv_0":                 ("wino4 wino4 wino4w", "wino2 wino4 wino4w", "wino2 wino4 wino4w"),
    "up_0.conv_1":                 ("wino4 wino4 wino4w", "wino2 wino4 wino4w", "wino2 wino4 wino4w"),
    "up_0.conv_s":                 ("direct direct direct", "direct direct direct", "direct direct direct"),
    "up_1.mlp_shared":             ("wino4 wino2 wino", "wino2 wino2 wino", "wino2 wino2 wino4w"),
    "up_1.gamma_beta[256]":        ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_1.gamma_beta[512]":        ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_1.conv_0":                 ("wino4 wino4 wino4w", "wino2 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_1.conv_1":                 ("wino4 wino4 wino4w", "wino2 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_1.conv_s":                 ("gemm gemm gemm_tn", "gemm gemm gemm_tn", "gemm gemm gemm_tn"),
    "up_2.mlp_shared":             ("wino4 wino4 wino", "wino4 wino2 wino", "wino4 wino4 wino4w"),
    "up_2.gamma_beta[128]":        ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_2.gamma_beta[256]":        ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_2.conv_0":                 ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_2.conv_1":                 ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_2.conv_s":                 ("gemm gemm gemm_tn", "gemm gemm gemm_tn", "gemm gemm gemm_tn"),
    "up_3.mlp_shared":             ("wino4 wino4 wino", "wino4 wino4 wino", "wino4 wino4 wino4w"),
    "up_3.gamma_beta[64]":         ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_3.gamma_beta[128]":        ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_3.conv_0":                 ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_3.conv_1":                 ("wino4 wino4 wino4w", "wino4 wino4 wino4w", "wino4 wino4 wino4w"),
    "up_3.conv_s":                 ("direct direct direct", "direct direct direct", "direct direct direct"),
    "conv_img":                    ("few few_direct few", "few few_direct few", "few few_direct few"),
    "D0.model0":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "D0.model1":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "D0.model2":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "D0.model3":                   ("direct wino34 direct", "direct wino34 direct", "direct wino34 direct"),
    "D0.model4":                   ("few few few", "few few few", "few few few"),
    "D1.model0":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "D1.model1":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "D1.model2":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "D1.model3":                   ("direct wino34 direct", "direct wino34 direct", "direct wino34 direct"),
    "D1.model4":                   ("few few few", "few few few", "few few few"),
    "objD.C4-64":                  ("direct direct direct", "direct direct direct", "direct direct direct"),
    "objD.C4-128":                 ("direct direct direct", "direct direct direct", "direct direct direct"),
    "objD.C4-256":                 ("direct direct direct", "direct direct direct", "direct direct direct"),
    "objD.fc":                     ("direct direct direct", "direct direct direct", "direct direct direct"),
    "objD.obj_classifier":         ("direct direct direct", "direct direct direct", "direct direct direct"),
    "objD.real_classifier":        ("direct direct direct", "direct direct direct", "direct direct direct"),
    "gconv0.net1.0":               ("direct direct direct", "direct direct direct", "direct direct direct"),
    "gconv.net1.0":                ("direct direct direct", "direct direct direct", "direct direct direct"),
    "gconv.net1.2":                ("direct direct direct", "direct direct direct", "direct direct direct"),
    "gconv.net2.0":                ("direct direct direct", "direct direct direct", "direct direct direct"),
    "gconv.net2.2":                ("direct direct direct", "direct direct direct", "direct direct direct"),
    "box_net.0":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
    "box_net.2":                   ("direct direct direct", "direct direct direct", "direct direct direct"),
}


@pytest.mark.parametrize("col,B,S,T,O", [(0, 16, 32, 16, 8), (1, 4, 32, 16, 8), (2, 6, 128, 16000, 128)])
def test_the_step_layers_keep_their_kernels(built, col, B, S, T, O):
    got = {name: _code(built.plan_conv(**kw, need=(True, True, True))) for name, kw in _rows(B, S, T, O)}
    assert got == {name: want[col] for name, want in STEP_PLANS.items()}


def test_planned_directions_follow_the_gradients_asked_for(built):
    """Only what `need` asks for is planned (no query for a direction that will not run); a forward pass nothing is
    differentiated through counts as backward-class (F(3x3,4x4) on the PatchGAN's 4x4 / stride 1 layer); the bias alone is
    a column sum."""
    g = dict(B=16, IH=33, IW=33, Cin=256, Cout=512, KH=4, KW=4, stride=1, pad=2, has_bias=True)
    assert _code(built.plan_conv(**g)) == "wino34 - -"
    assert _code(built.plan_conv(**g, need=(False, False, True))) == "wino34 - colsum"
    assert _code(built.plan_conv(**g, need=(False, True, False))) == "direct - direct"
    assert _code(built.plan_conv(**g, need=(True, False, False))) == "direct wino34 -"


def test_call_options(built):
    """One row per conv2d option: dx_range, frozen packs (which never take F(3x3,4x4)), in_act, pre_slope, cout_real 1..3."""
    need = (True, True, True)
    rows = [
        (dict(B=16, IH=256, IW=256, Cin=40, Cout=64, KH=4, KW=4, stride=2, pad=2, act=LEAKY, dx_range=(0, 32)),
         "direct range direct"),
        (dict(B=16, IH=64, IW=64, Cin=256, Cout=256, KH=3, KW=3, stride=1, pad=1, act=LEAKY, packs=True), "wino4 wino4 wino4w"),
        (dict(B=16, IH=33, IW=33, Cin=256, Cout=512, KH=4, KW=4, stride=1, pad=2, packs=True), "direct direct direct"),
        (dict(B=16, IH=16, IW=16, Cin=128, Cout=64, KH=3, KW=3, stride=1, pad=1, in_act=(LEAKY, 0.2)), "wino2 wino2 wino4w"),
        (dict(B=16, IH=256, IW=256, Cin=64, Cout=4, KH=3, KW=3, stride=1, pad=1, act=TANH, cout_real=3, pre_slope=0.2),
         "few few_direct few"),
        (dict(B=16, IH=33, IW=33, Cin=512, Cout=1, KH=4, KW=4, stride=1, pad=2, cout_real=1), "few few few"),
        (dict(B=4, IH=32, IW=32, Cin=64, Cout=2, KH=3, KW=3, stride=1, pad=1, cout_real=2), "few few_direct few"),
        (dict(B=16, IH=256, IW=256, Cin=64, Cout=3, KH=3, KW=3, stride=1, pad=1, act=TANH, cout_real=3), "few few_direct few"),
    ]
    for kw, want in rows:
        assert _code(built.plan_conv(**kw, has_bias=True, need=need)) == want, kw
    few = built.plan_conv(**rows[4][0], need=need).few
    assert (few.cout_real, few.in_act, few.in_slope) == (3, 1, pytest.approx(0.2))
    with pytest.raises(RuntimeError, match="pre_slope is served by the few-output kernels only"):
        built.plan_conv(16, 32, 32, 64, 64, 3, 3, 1, 1, pre_slope=0.2)
    with pytest.raises(RuntimeError, match="pre_slope with >= 256 input channels is not served"):
        built.plan_conv(16, 33, 33, 512, 1, 4, 4, 1, 2, cout_real=1, pre_slope=0.2, need=need)
    with pytest.raises(RuntimeError, match="not a multiple of 4 reached the kernels"):
        built.plan_conv(16, 32, 32, 64, 6, 3, 3, 1, 1)


def test_variant_follows_the_grid(built):
    """F(4x4,3x3) on launches that fill the chip, F(2x2,3x3) where fewer than ~160 (region, channel block) items would leave
    it half idle — unless the launch is plain and long enough to be split over its input channels."""
    ops = built
    assert ops.wino_variant(16, 64, 64, 512, 256) == 4            # 512 items
    assert ops.wino_variant(4, 64, 64, 512, 256) == 2             # 128 items, epilogue: not splittable
    assert ops.wino_variant(4, 64, 64, 512, 256, plain=True) == 4     # split over 512 input channels instead
    assert ops.wino_variant(4, 32, 32, 128, 512, plain=True) == 2     # 64 items, too few channels to split
    assert ops.wino_variant(6, 64, 64, 256, 256) == 4             # 192 items
    assert ops.wino_variant(4, 16, 16, 512, 512) == 2             # below 32 pixels: never F(4x4,3x3)


def test_winograd_split_and_slice_rules_hold_at_their_boundaries(built):
    """The host rules csrc/csg_wino_host.h holds once, as the C ABI's size functions report them: the split over the input
    channels (under 384 blocks, cut towards 512; F(2x2,3x3): from 16 stages of 16 channels, 8 per range; F(4x4,3x3) and
    F(3x3,4x4): from 32 stages of 8 channels, 16 per range), the slices of the two weight gradients (1024 blocks, >= 8 regions,
    <= 512 slices; 256 blocks, >= 16 regions, <= 256 slices, two slabs per slice) and the pack sizes (16 | 36 positions).  Every
    expected value is the answer of the library before these rules were shared; each sits where one constant decides it."""
    from canonicalsg2im_amd._lib import lib
    ops = built

    def d(B, H, W, Cin, Cout, act=NONE):
        return ops._wino_desc(B, H, W, Cin, Cout, act, 0.2 if act else 0.0)

    f2 = {(1, 32, 32, 2048, 128): 8388608,          # 2 blocks, 128 stages: 16 ranges of 8 stages
          (1, 32, 32, 256, 128): 1048576,           # 16 stages: the fewest that split, 2 ranges
          (1, 32, 32, 240, 128): 0,                 # 15 stages
          (2, 64, 64, 256, 256): 16777216,          # 256 blocks: 2 ranges
          (3, 64, 64, 256, 256): 0,                 # 384 blocks fill the chip
          (1, 8, 8, 2048, 128): 524288,             # 4 x 4 tile regions
          (383, 8, 8, 256, 64): 12550144,           # 383 blocks still split
          (7, 8, 8, 9472, 64): 8486912,             # 7 blocks: ceil(512 / 7) = 74 ranges (511 would give 73)
          (2, 64, 64, 640, 128): 16777216}          # 128 blocks: 512 / 128 = 4 ranges (513 would give 5)
    for k, want in f2.items():
        assert lib.csg_wino_conv_workspace(d(*k)) == want, k
    assert lib.csg_wino_conv_workspace(d(1, 32, 32, 2048, 128, LEAKY)) == 0        # an epilogue: never split
    f4 = {(1, 32, 64, 256, 64): 1048576,            # 32 stages: the fewest that split
          (1, 32, 64, 248, 64): 0,                  # 31 stages
          (1, 32, 64, 512, 64): 2097152,            # 64 stages: 4 ranges of 16
          (1, 32, 64, 480, 64): 1572864,            # 60 stages: 3 ranges (15 per range would give 4)
          (4, 64, 64, 512, 256): 67108864,          # 128 blocks: ceil(512 / 128) = 4 ranges
          (6, 64, 64, 512, 256): 75497472,          # 192 blocks: 3 ranges
          (1, 16, 16, 512, 64): -1}                 # narrower than 32 pixels: refused
    for k, want in f4.items():
        assert lib.csg_wino4_conv_workspace(d(*k)) == want, k
    f34 = {(1, 31, 31, 512, 64): (921600, 1048576),          # 30 x 30 | 32 x 32 outputs, 64 stages: 4 ranges
           (1, 31, 31, 256, 64): (460800, 524288),           # 32 stages
           (1, 31, 31, 248, 64): (0, 0),                     # 31 stages
           (2, 63, 63, 512, 512): (31490048, 33554432),
           (16, 31, 31, 512, 512): (0, 0)}                   # 1152 blocks
    for k, want in f34.items():
        assert (lib.csg_wino34_conv_workspace(d(*k), 1), lib.csg_wino34_conv_workspace(d(*k), 2)) == want, k
    wg = {(1, 8, 8, 64, 64): (147712, 295424),               # one slice: one slab | its two halves
          (1, 32, 32, 128, 128): (1180672, 1180672),         # 16 regions: 2 slices of 8 | 1 slice of 16
          (4, 64, 64, 256, 128): (37765120, 37765120),       # 256 regions: 32 slices of 8 | 16 slices of 16, x 2
          (1, 12, 12, 64, 64): (-1, -1),                     # neither stage tiles the image
          (1, 24, 40, 64, 64): (-1, 295424),                 # 8 x 8-pixel stages do, 16 x 2-tile stages do not
          (31, 8, 8, 64, 64): (590848, 590848),              # 31 regions: 4 slices (7 per slice: 5) | 2 x 2 (15: 3)
          (33, 8, 8, 64, 64): (738560, 886272),              # 33 regions: 5 slices (9 per slice: 4) | 3 x 2 (17: 2)
          (16, 64, 64, 256, 128): (75530240, 37765120),      # the block targets decide: 1024 / 16 = 64 | 256 / 16 = 16, x 2
          (4, 256, 256, 96, 64): (75732480, 28344320),       # ceil(1024 / 3) = 342 slices (1023: 341) | 256 / 4 = 64, x 2
          (5, 256, 256, 32, 64): (37879808, 18939904)}       # at most 512 slices | 256 / 2 = 128, x 2
    for k, want in wg.items():
        assert (lib.csg_wino_bwd_weight_workspace(d(*k)), lib.csg_wino4_bwd_weight_workspace(d(*k))) == want, k
    packs = {(1, 1): (16384, 36864), (33, 9): (65536, 147456), (128, 2048): (16777216, 37748736), (0, 8): (-1, -1)}
    for k, want in packs.items():
        assert (lib.csg_wino_pack_bytes(*k), lib.csg_wino4_pack_bytes(*k)) == want, k
    # the variant rule asks that same planner: 128 items stay on F(4x4,3x3) from the 32 stages that split
    assert ops.wino_variant(4, 64, 64, 248, 256, plain=True) == 2
    assert ops.wino_variant(4, 64, 64, 256, 256, plain=True) == 4


def test_default_rule_sends_the_narrow_shortcuts_to_the_gemm_kernels(built):
    """Mode "auto" (the default): N <= 256 <= K with at least 256 tiles — conv_s of the 64 x 64 and 128 x 128 residual blocks
    at batch 16; the graph encoder's wide linears and everything small stay on the implicit-GEMM kernel."""
    ops = built
    old, ops.GEMM_MODE = ops.GEMM_MODE, "auto"
    try:
        assert ops.gemm_eligible(16 * 128 * 128, 128, 256) and ops.gemm_eligible(16 * 64 * 64, 256, 512)
        assert not ops.gemm_eligible(96000, 512, 384) and not ops.gemm_eligible(96000, 1152, 512)
        assert not ops.gemm_eligible(768, 128, 512) and not ops.gemm_eligible(16 * 256 * 256, 64, 128)
    finally:
        ops.GEMM_MODE = old


def test_unsupported_shapes_are_declined(built):
    from canonicalsg2im_amd._lib import FewDesc, lib
    d = FewDesc()
    d.B, d.IH, d.IW, d.Cin, d.x_cs, d.KH, d.KW, d.pad, d.cout_real, d.act, d.slope = 1, 8, 8, 64, 64, 5, 5, 2, 1, 0, 0.0
    assert lib.csg_conv_few_supported(d) == 0                       # 5x5
    d.KH = d.KW = 4
    d.cout_real = 3
    assert lib.csg_conv_few_supported(d) == 0                       # 16 taps x 3 outputs: registers
    d.cout_real, d.Cin, d.x_cs = 1, 48, 48
    assert lib.csg_conv_few_supported(d) == 0                       # Cin not a power-of-two multiple of 32


def test_wino_weight_gradient_workspace_refuses_images_its_stages_do_not_tile(built):
    """The F(3x3,2x2) weight-gradient kernel stages 16 tiles (16x1, 8x2 or 4x4) at a time and wants them to tile the image
    exactly; other sizes are refused by the C ABI (the plan then keeps the direct kernel)."""
    from canonicalsg2im_amd._lib import WinoDesc, lib
    for (H, W, ok) in ((12, 20, False), (24, 40, False), (6, 130, False), (8, 8, True), (4, 16, True), (2, 64, True)):
        d = WinoDesc()
        d.B, d.H, d.W, d.Cin, d.x_cs, d.Cout, d.y_cs, d.act, d.slope = 1, H, W, 16, 16, 32, 32, 0, 0.0
        assert (lib.csg_wino_bwd_weight_workspace(d) >= 0) == ok, (H, W)
    assert built.plan_conv(20, 24, 40, 16, 32, 3, 3, 1, 1, need=(False, True, False)).wgrad == "direct"
