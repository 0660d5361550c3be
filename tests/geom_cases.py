"""The geometry path matrix: one row per code path (and per kernel corner) of csrc/layout.hip and csrc/crop.hip that the
public entry points can reach, with `geom_ref64`, a plain float64 CPU restatement of the family's contract (reference
sg2im/layout.py:12-188, sg2im/bilinear.py:44-94, discriminator.py:102-120).  Used by tests/test_gpu_geom_paths.py (each
row through the entry point it names on the device) and tests/test_geom_cases.py (on the CPU: the reference against the
oracle and against F.grid_sample, the table's coverage, the rows' distance from every discontinuity).

A row (dict, built by `row`) holds
  name, family    — the id; "layout" | "crop"
  entry           — "layout_pyramid" | "disc_input" | "layout_paint" (ops.*), "abi_slice" (csg_layout_fwd / csg_layout_bwd
                    called with a channel slice of a wider buffer) or "crop_objects"
  layout rows     — B, O, S; H, W: the full-resolution layout; sizes: the (h, w) of every output level
  crop rows       — B, C, H, W: the images; N crops of HH x HH; idx: how `img_idx` is laid out ("sorted" | "unsorted": a
                    permutation that also leaves image 1 without a crop)
  masks           — None | ("int" | "soft", M): (O, M, M) int64 / float32 masks (masks_to_layout)
  boxes           — the box family (BOX_FAMILIES below)
  valid           — "all" | "gaps" (every third object masked out) | "ragged" (image b loses its last 2 b + 1 objects) |
                    "img1_none" (image 1 has no valid object)
  need            — what requires grad, a subset of ("vecs", "boxes", "masks", "img")
  img_fmt         — disc_input: "nchw" | "cl" (channels-last image)
  out_cs, out_off — abi_slice: pixel stride of the wider buffer and the slice's first channel
  kernels         — what the dispatch rules give for the row, COMPUTED by `level_rule` / `_kernel_names` (restatements of
                    layout_fwd_launch, layout_bwd_tiled, the bd choice and _CropObjects); one string per level,
                    "<forward kernel>[+blk]x<chunks>/<backward to vecs>"
  refuse          — the call must raise a RuntimeError matching this pattern before any launch
  seed            — added to the data generator's seed (crc32 of the name): moved when the fp64 reference alone finds the
                    row too close to a discontinuity (tests/test_geom_cases.py: conditions (a), (b), (c))

No row excludes anything from its comparison: the inputs are chosen so that no contributing sample sits where float32 and
float64 disagree about a bilinear cell, no two paint masses are close and no sampled mask is close to the 0.5 threshold.
Zero-size boxes are out of scope (the reference divides by the size)."""
import zlib

import torch
import torch.nn.functional as F

# csrc/layout.hip:118-121,421 and csrc/crop.hip:90-91
LAY_OB, LAY_CULL, LAY_PXC, LAY_EPT, LAY_BB, LAY_ROWS = 32, 256, 256, 8, 8, 4
CROP_MAXHW, CROP_K, CROP_TILE = 64, 8, 16
BOX_FAMILIES = ("inside", "border", "outside", "full", "thin", "reversed", "mixed")
MIXED = ("inside", "border", "outside", "full", "thin", "reversed")
PAINT_MASS_GAP, PAINT_THRESHOLD_GAP = 1e-3, 1e-4
SENTINEL = -777.25           # abi_slice: what the wider buffer holds outside the slice


def cdiv(a, b):
    return -(-a // b)


def hw(size):
    return (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size), int(size))


# ------------------------------------------------------------------------------------------------- the dispatch rules
def level_rule(S, OH, OW, O, masks, dboxes, need_vecs=True):
    """What serves one output level.  Forward: layout_fwd_launch (csrc/layout.hip:951-970); backward to vecs (and boxes):
    layout_bwd_tiled (:974-985), else the one-block kernel with bd (:1052-1053)."""
    qpp = S // 4
    pxc = min((LAY_EPT * 256) // qpp, LAY_PXC, OW)                                       # :952-954
    blocked = 256 % qpp == 0 and pxc % LAY_EPT == 0                                      # :162, :958
    rows = masks is None and blocked and OH >= 32                                        # :958
    lds = (LAY_OB * pxc + LAY_OB * S) * 4 + ((LAY_CULL * LAY_ROWS + LAY_CULL) if rows else 4 * LAY_CULL) * 4 + 16  # :956,961
    r = dict(fwd="rows" if rows else "plain", blocked=blocked, pxc=pxc, chunks=cdiv(OW, pxc), lds=lds, bwd=None, npl=None,
             ntiles=0)
    if need_vecs or dboxes:
        tiled = (masks is None and not dboxes and O > 0 and qpp <= 256 and 256 % qpp == 0 and OH >= 32 and
                 pxc % LAY_EPT == 0)                                                     # :976-982
        if tiled:
            r.update(bwd="tiled", ntiles=cdiv(OW, pxc) * cdiv(OH, LAY_ROWS))             # :983
        else:
            bd = 1024 if OH * OW >= 64 * 64 else 256                                     # :1052
            r.update(bwd="bd%d" % bd, npl=bd // qpp)                                     # :1053
    return r


def level_rules(c):
    if c["entry"] == "layout_paint":
        return []
    return [level_rule(c["S"], h, w, c["O"], c["masks"], "boxes" in c["need"], bool(set(c["need"]) & {"vecs", "boxes"}))
            for (h, w) in c["sizes"]]


def _kernel_names(c):
    if c["family"] == "crop":                               # _CropObjects (ops.py): csg_crop_fwd, then one kernel per gradient
        return ("crop_fwd",) + (("crop_bwd",) if "img" in c["need"] else ()) + (("crop_bwd_boxes",) if "boxes" in c["need"] else ())
    if c["entry"] == "layout_paint":
        return ("mass", "paint")
    out = tuple("%s%sx%d/%s" % (r["fwd"], "+blk" if r["blocked"] else "", r["chunks"], r["bwd"]) for r in level_rules(c))
    return out + (("bwd_masks",) if "masks" in c["need"] else ())


def row(name, entry, B=2, O=6, S=32, H=32, W=None, sizes=None, masks=None, boxes="inside", valid="all", need=("vecs",),
        C=3, N=0, HH=8, idx="sorted", img_fmt="nchw", out_cs=None, out_off=0, refuse=None, seed=0):
    family = "crop" if entry == "crop_objects" else "layout"
    assert boxes in BOX_FAMILIES and entry in ("layout_pyramid", "disc_input", "layout_paint", "abi_slice", "crop_objects")
    W = H if W is None else W
    sizes = tuple(hw(s) for s in (sizes if sizes is not None else [(H, W)]))
    c = dict(name=name, family=family, entry=entry, B=B, O=O, S=S, H=H, W=W, sizes=sizes, masks=masks, boxes=boxes, valid=valid,
             need=tuple(need), C=C, N=N, HH=HH, idx=idx, img_fmt=img_fmt, out_cs=out_cs, out_off=out_off, refuse=refuse,
             seed=seed)
    if entry == "disc_input":
        assert sizes == ((H, H),) and W == H
    if entry == "abi_slice":
        assert len(sizes) == 1 and out_cs >= out_off + S
    c["kernels"] = _kernel_names(c)
    return c


LP, DI, PT, AB, CR = "layout_pyramid", "disc_input", "layout_paint", "abi_slice", "crop_objects"
VB, VBM, ALLG = ("vecs", "boxes"), ("vecs", "boxes", "masks"), ("img", "vecs", "boxes", "masks")

CASES = [
    # ---- forward kernels and thread maps; backward to vecs: tiled and one-block, and their sum over a pyramid
    # S = 8: OW = 320 is two chunks of 256 + 64; OH = 34 leaves two rows in the last ROWS block; (8, 320) is the plain kernel
    # on the same chunks; (2, 36): 36 % 8 != 0 -> the unblocked map.  Tiled + bd256 + bd256 accumulate into one dvecs.
    row("lay_s8_34x320", LP, O=12, S=8, H=34, W=320, sizes=[(34, 320), (8, 320), (2, 36)]),
    row("lay_s12_64", LP, O=10, S=12, sizes=[64, 32], H=64),                  # S/4 = 3: unblocked at OH >= 32; bd1024, bd256
    row("lay_s20_31x40", LP, O=8, S=20, H=31, W=40),                          # S/4 = 5; OH = 31: one row short of ROWS blocks
    row("lay_s32_64", LP, O=10, S=32, H=64, sizes=[64, 32, 16, 8]),           # the trainer's pyramid: rows, rows, plain, plain
    row("lay_s32_34x36", LP, O=8, S=32, H=34, W=36),                          # OW = 36 falls off the blocked path at OH >= 32
    row("lay_s32_24x40", LP, O=8, S=32, H=24, W=40, sizes=[(24, 40), (12, 20)]),
    row("lay_s40_64x48", LP, O=8, S=40, H=64, W=48, sizes=[(64, 48), (32, 24)]),
    row("lay_s128_64x128", LP, O=10, S=128, H=64, W=128, sizes=[(64, 128), (32, 64)]),   # config C5: pxc = 64, two chunks
    row("lay_s512_32", LP, O=6, S=512, H=32, sizes=[32, 8]),                  # more than 64 KB of dynamic LDS; npl = 2
    row("lay_s1024_32", LP, O=6, S=1024, H=32, sizes=[32, 8]),                # about 134 KB; pxc = 8; one-block npl = 1
    # ---- object counts
    row("lay_o0", LP, O=0, S=32, H=32),
    row("lay_o1", LP, O=1, S=32, H=32, need=VB),
    row("lay_full33", LP, O=33, S=32, H=64, sizes=[64, 16], boxes="full"),    # 33 survivors per tile: second staging group
    row("lay_full33_s12", LP, O=33, S=12, H=32, boxes="full"),                # the same on the unblocked map
    row("lay_full33_db", LP, O=33, S=8, H=32, boxes="full", need=VB),
    row("lay_o300_gaps", LP, O=300, S=32, H=64, sizes=[64, 16], valid="gaps"),   # second culling pass
    row("lay_img1_none", LP, B=3, O=5, S=32, H=32, valid="img1_none", need=VB),
    # ---- box families, forward and backward to the boxes (one-block kernel, both block sizes, two levels accumulate)
    row("lay_db_inside", LP, O=10, S=32, H=64, sizes=[64, 32], need=VB),
    row("lay_db_border", LP, O=8, S=8, H=64, sizes=[64, 16], boxes="border", need=VB),
    row("lay_db_thin", LP, O=8, S=8, H=32, boxes="thin", need=VB),
    row("lay_db_mixed", LP, O=12, S=12, H=64, W=48, boxes="mixed", valid="ragged", need=VB),
    row("lay_db_outside", LP, O=4, S=8, H=32, boxes="outside", need=VB),
    row("lay_db_reversed", LP, O=6, S=8, H=64, boxes="reversed", need=VB),
    row("lay_border_tiled", LP, O=12, S=32, H=64, boxes="border"),            # the x cull of the rows / tiled kernels
    row("lay_thin_tiled", LP, O=12, S=32, H=64, W=128, boxes="thin"),
    row("lay_mixed_tiled", LP, O=18, S=128, H=32, W=128, boxes="mixed"),      # two chunks: objects culled per chunk
    # ---- masks: forward, backward to vecs / boxes / masks (accumulating over the levels)
    row("lay_m16_int", LP, O=6, S=32, H=64, sizes=[64, 32], masks=("int", 16), need=VB),
    row("lay_m16_int_24x40", LP, O=6, S=8, H=24, W=40, sizes=[(24, 40), (12, 20)], masks=("int", 16), need=VB),
    row("lay_m32_soft_24x40", LP, O=6, S=8, H=24, W=40, sizes=[(24, 40), (12, 20)], masks=("soft", 32), need=VBM),
    row("lay_m16_soft_border", LP, O=8, S=12, H=32, sizes=[32, 16], masks=("soft", 16), boxes="border", need=VBM),
    # thin boxes under a mask: d weight / d t = M / size = 16 * 31 / 0.3, so the 3e-8 by which float32 pixel centres differ
    # from linspace's true values would be 5e-5 of the output.  33 pixels: the centres k / 32 are exact in both precisions.
    row("lay_m16_int_thin", LP, O=8, S=8, H=33, masks=("int", 16), boxes="thin", need=VB),
    row("lay_m1_soft_mixed", LP, O=12, S=8, H=64, masks=("soft", 1), boxes="mixed", valid="gaps", need=VBM),
    row("lay_m32_soft_s128", LP, O=4, S=128, H=32, sizes=[32, 16], masks=("soft", 32), need=VBM),
    row("lay_m16_full33", LP, O=33, S=8, H=32, masks=("soft", 16), boxes="full", need=("vecs", "masks")),
    # ---- the discriminator's packed input [layout | img | 0]
    row("disc_s8", DI, O=6, S=8, H=32, need=("img", "vecs")),
    row("disc_s12_cl", DI, O=6, S=12, H=64, img_fmt="cl", need=("img", "vecs", "boxes")),
    row("disc_s32_cl", DI, O=8, S=32, H=64, img_fmt="cl", valid="ragged", need=("img", "vecs")),
    row("disc_s32_border", DI, O=8, S=32, H=34, boxes="border", need=("img", "vecs", "boxes")),
    row("disc_s128", DI, O=8, S=128, H=32, need=("vecs",)),
    row("disc_s32_m16_int", DI, O=6, S=32, H=64, masks=("int", 16), img_fmt="cl", need=("img", "vecs", "boxes")),
    row("disc_s8_m1_soft", DI, O=6, S=8, H=32, masks=("soft", 1), valid="gaps", need=ALLG),
    row("disc_s12_m32_soft", DI, O=5, S=12, H=32, masks=("soft", 32), need=ALLG),
    row("disc_s128_m16_soft", DI, O=4, S=128, H=32, masks=("soft", 16), img_fmt="cl", need=("vecs", "masks")),
    # ---- a channel slice of a wider buffer (the C ABI's out_cs / out_off)
    row("abi_off4_plain", AB, O=6, S=8, H=16, out_cs=16, out_off=4, need=VB),
    row("abi_off36_rows", AB, O=8, S=32, H=32, out_cs=72, out_off=36),
    row("abi_off36_s12", AB, O=8, S=12, H=64, out_cs=52, out_off=36, boxes="border", need=VB),
    row("abi_off4_m16", AB, O=5, S=8, H=32, sizes=[(16, 16)], out_cs=20, out_off=4, masks=("soft", 16), need=VB),
    # ---- test mode: the painter's compositing
    row("paint_int_m16", PT, O=6, S=32, H=32, sizes=[32, 16], masks=("int", 16), need=()),
    row("paint_soft_m32_24x40", PT, B=3, O=5, S=8, H=24, W=40, sizes=[(24, 40), (12, 20)], masks=("soft", 32),
        valid="ragged", need=(), seed=1),
    row("paint_soft_m1", PT, O=6, S=12, H=32, sizes=[32, 8], masks=("soft", 1), valid="gaps", need=()),
    row("paint_int_m1_48x32", PT, B=1, O=4, S=8, H=48, W=32, sizes=[(48, 32), (24, 16)], masks=("int", 1), boxes="border",
        need=()),
    row("paint_int_m32_img1_none", PT, B=3, O=4, S=8, H=33, sizes=[33, 16], masks=("int", 32), valid="img1_none", need=()),
    # ---- object crops
    row("crop_c3_64", CR, B=2, C=3, H=64, N=10, HH=32, need=("img", "boxes")),
    row("crop_c1_40x72", CR, B=2, C=1, H=40, W=72, N=8, HH=8, boxes="border", need=("img", "boxes")),
    row("crop_c4_17x129", CR, B=2, C=4, H=17, W=129, N=6, HH=64, need=("img", "boxes")),
    row("crop_hh1", CR, B=2, C=3, H=64, N=6, HH=1, need=("img", "boxes")),
    row("crop_n0", CR, B=2, C=3, H=64, N=0, HH=8, need=("img",)),
    row("crop_n1", CR, B=2, C=3, H=64, N=1, HH=8, need=("img", "boxes")),
    row("crop_n300", CR, B=2, C=3, H=64, N=300, HH=8, need=("img",)),         # second candidate pass; > CROP_K per tile
    row("crop_full12", CR, B=1, C=3, H=40, W=72, N=12, HH=32, boxes="full", need=("img", "boxes")),   # 12 crops on every tile
    row("crop_unsorted_skip", CR, B=3, C=3, H=64, N=9, HH=8, idx="unsorted", need=("img", "boxes")),
    row("crop_outside", CR, B=2, C=3, H=64, N=4, HH=8, boxes="outside", need=("img", "boxes")),
    row("crop_thin", CR, B=2, C=3, H=40, W=72, N=8, HH=32, boxes="thin", need=("img", "boxes")),       # slope <= 1e-3
    row("crop_reversed", CR, B=2, C=4, H=64, N=6, HH=8, boxes="reversed", need=("img", "boxes")),
    row("crop_mixed", CR, B=2, C=3, H=17, W=129, N=12, HH=8, boxes="mixed", need=("img", "boxes")),
    row("crop_small_slope", CR, B=1, C=3, H=64, N=4, HH=64, boxes="inside", need=("img",), seed=100),  # widest windows
    row("crop_fwd_c8", CR, B=2, C=8, H=32, N=4, HH=8, need=()),
    row("crop_fwd_hh96", CR, B=2, C=3, H=64, N=3, HH=96, need=()),
    row("refuse_crop_c8", CR, B=2, C=8, H=32, N=4, HH=8, need=("img",), refuse="at most 4 image channels"),
    row("refuse_crop_hh96", CR, B=2, C=3, H=64, N=3, HH=96, need=("boxes",), refuse="64 x 64 crops"),
]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


# ------------------------------------------------------------------------------------------------- data
def _f32(t):
    """Values every precision can hold: the inputs of a row are float32 numbers."""
    return t.to(torch.float32).to(torch.float64)


def _axis(fam, g, n_px, n_src, thin):
    """(lo, size) of one box along one axis of n_px pixel centres, sampled from an n_src-pixel source."""
    u = lambda a, b: a + (b - a) * float(torch.rand((), generator=g, dtype=torch.float64))
    if fam == "inside":
        size = u(0.15, 0.45)
        return u(0.03, 0.97 - size), size
    if fam == "border_lo":                       # overhangs the low edge: lo < 0
        size = u(0.25, 0.5)
        return u(-0.4 * size, -0.1 * size), size
    if fam == "border_hi":                       # lo + size > 1
        size = u(0.25, 0.5)
        return 1.0 - u(0.6, 0.9) * size, size
    if fam == "outside":                         # the whole support (size / (2 n) beyond the box) is off the image
        size = u(0.1, 0.3)
        return (u(1.2, 1.6), size) if u(0, 1) < 0.5 else (u(-0.9, -0.5), size)
    if fam == "full":
        return 0.0, 1.0
    if fam == "thin" and thin:                   # 0.3 pixel pitches wide, around the centre of pixel k
        size = 0.3 / (n_px - 1)
        k = int(u(2, n_px - 2))
        t = float(torch.linspace(0, 1, n_px, dtype=torch.float32)[k])
        return t - size * u(0.35, 0.65), size
    if fam == "reversed" and thin:               # negative size: the box runs from lo down to lo + size
        size = -u(0.2, 0.45)
        return u(0.55, 0.95), size
    return _axis("inside", g, n_px, n_src, False)


def _box(fam, o, g, H, W, n_src):
    """One [x0, y0, w, h] of the family; `o` picks the edge / the thin or reversed axis."""
    if fam == "mixed":
        fam = MIXED[o % len(MIXED)]
        o //= len(MIXED)
    if fam == "border":
        edge = o % 4                             # left, right, top, bottom; every fourth object takes a corner too
        fx = ("border_lo", "border_hi", "inside", "inside")[edge]
        fy = ("inside", "inside", "border_lo", "border_hi")[edge]
        if o % 8 >= 4:
            fy = "border_hi" if edge < 2 else fy
            fx = "border_lo" if edge >= 2 else fx
        (x0, w), (y0, h) = _axis(fx, g, W, n_src, True), _axis(fy, g, H, n_src, True)
    elif fam == "reversed":                      # negative width (every third object: negative height too)
        (x0, w), (y0, h) = _axis(fam, g, W, n_src, True), _axis(fam, g, H, n_src, o % 3 == 2)
    elif fam == "thin":                          # thin in x, in y, in both
        (x0, w), (y0, h) = _axis(fam, g, W, n_src, o % 3 != 1), _axis(fam, g, H, n_src, o % 3 != 0)
    else:
        (x0, w), (y0, h) = _axis(fam, g, W, n_src, True), _axis(fam, g, H, n_src, True)
    return [x0, y0, w, h]


def _crop_thin_axis(g, n_px, HH):
    """A crop axis whose grid slope size * n_px / (HH - 1) is 6e-4 source pixels per crop pixel (the scan-everything branch
    of k_crop_bwd, csrc/crop.hip:159-166), all of it inside one bilinear cell."""
    u = lambda a, b: a + (b - a) * float(torch.rand((), generator=g, dtype=torch.float64))
    size = 6e-4 * max(HH - 1, 1) / n_px
    k = int(u(1, n_px - 2))
    return (k + 0.5 + u(0.25, 0.6)) / n_px, size          # f = lo * n_px - 1/2 in [k + 0.25, k + 0.65)


def _valid(c):
    B, O = c["B"], c["O"]
    v = torch.ones(B, O, dtype=torch.bool)
    if c["valid"] == "gaps":
        v[:, 1::3] = False
    elif c["valid"] == "ragged":
        for b in range(B):
            v[b, max(O - (2 * b + 1), 0):] = False
    elif c["valid"] == "img1_none":
        v[1] = False
    return v


def make_data(c):
    """The row's inputs and incoming gradients, float64 CPU tensors holding float32 values (masks: int64 for "int")."""
    g = torch.Generator().manual_seed((zlib.crc32(c["name"].encode()) + c["seed"]) & 0x7FFFFFFF)
    rn = lambda *s: _f32(torch.randn(*s, generator=g, dtype=torch.float64))
    B, H, W = c["B"], c["H"], c["W"]
    if c["family"] == "crop":
        C, N, HH = c["C"], c["N"], c["HH"]
        boxes = []
        for n in range(N):
            if c["boxes"] == "thin" or (c["boxes"] == "mixed" and MIXED[n % len(MIXED)] == "thin"):
                k = n // len(MIXED) if c["boxes"] == "mixed" else n
                ax = _crop_thin_axis(g, W, HH) if k % 3 != 1 else _axis("inside", g, W, W, False)
                ay = _crop_thin_axis(g, H, HH) if k % 3 != 0 else _axis("inside", g, H, H, False)
                boxes.append([ax[0], ay[0], ax[1], ay[1]])
            else:
                boxes.append(_box(c["boxes"], n, g, H, W, W))
        boxes = _f32(torch.tensor(boxes, dtype=torch.float64).reshape(N, 4))
        if c["idx"] == "sorted":
            idx = (torch.arange(N) * B) // max(N, 1)
        else:                                    # a permutation; image 1 has no crop
            pool = torch.tensor([b for b in range(B) if b != 1])
            idx = pool[torch.randint(0, len(pool), (N,), generator=g)]
        Cp = (C + 3) // 4 * 4
        # A sample coordinate on a 129-pixel axis carries 129 * 2^-24 = 8e-6 pixels of float32 rounding however it is
        # computed; times the neighbour differences of a white-noise image (up to 2 x its largest entry) that alone is the
        # 1e-5 gate.  So the image is a level per (image, channel) plus noise of 0.3 and the incoming gradient has mean 1:
        # the rounding term stays a third of the gate, a wrong or missing tap still costs a tenth of the scale.
        level = _f32(torch.rand(B, C, 1, 1, generator=g, dtype=torch.float64) + 1.5) * (1 - 2 * (torch.arange(C) % 2)).view(1, C, 1, 1)
        return dict(img=_f32(level + 0.3 * rn(B, C, H, W)), boxes=boxes, img_idx=idx.to(torch.int64),
                    dout=_f32(1 + rn(N, Cp, HH, HH)))
    O, S = c["O"], c["S"]
    M = c["masks"][1] if c["masks"] else 8
    boxes = _f32(torch.tensor([[_box(c["boxes"], o, g, H, W, M) for o in range(O)] for _ in range(B)],
                              dtype=torch.float64).reshape(B, O, 4))
    d = dict(vecs=rn(B, O, S), boxes=boxes, valid=_valid(c), masks=None)
    if c["masks"]:
        kind, M = c["masks"]
        r = torch.rand(B, O, M, M, generator=g, dtype=torch.float64)
        d["masks"] = (r > (0.35 if M > 1 else -1.0)).to(torch.int64) if kind == "int" else _f32(r)   # (a 1 x 1 int mask: 1)
    if c["entry"] == "disc_input":
        Ct = (S + 3 + 3) // 4 * 4
        d["img"] = rn(B, 3, H, H)
        d["douts"] = [rn(B, Ct, H, H)]
    else:
        d["douts"] = [rn(B, S, h, w) for (h, w) in c["sizes"]]
    return d


# ------------------------------------------------------------------------------------------------- geom_ref64
def src_index(n_out, n_full):
    """Nearest level: output index i reads full-resolution index floor(i * n_full / n_out)."""
    return torch.clamp((torch.arange(n_out) * n_full) // n_out, max=n_full - 1)


def axis_ix(lo, size, n_full, n_src, idx=None):
    """(O, n): the un-normalised sample coordinate of every pixel centre along one axis — _boxes_to_grid (layout.py:98-110)
    then grid_sample's align_corners=False unnormalisation, in ATen's order of operations (the order the kernels' comments
    restate: csrc/layout.hip:26-28)."""
    t = torch.linspace(0, 1, steps=n_full, dtype=lo.dtype)
    if idx is not None:
        t = t[idx]
    g = ((t.view(1, -1) - lo.view(-1, 1)) / size.view(-1, 1)) * 2 - 1
    return ((g + 1) * n_src - 1) / 2


def tap_matrix(ix, n_src):
    """(..., n_src): the bilinear weights each sample puts on the n_src source pixels (zeros padding: taps outside the
    source get nothing).  floor() carries no gradient; the fraction does: what ATen's grid_sampler backward computes."""
    i0 = torch.floor(ix).detach()
    fr = (ix - i0).unsqueeze(-1)
    m = torch.arange(n_src, dtype=ix.dtype)
    i0 = i0.unsqueeze(-1)
    return (m == i0).to(ix.dtype) * (1 - fr) + (m == i0 + 1).to(ix.dtype) * fr


def layout_ref64(vecs, boxes, masks, H, W, sizes):
    """One image, its valid objects: [(S, h, w)] — sum_o vec[o] x weight[o] with weight separable for boxes_to_layout
    (a constant 8-pixel source) and a bilinear sample of the (M, M) mask for masks_to_layout."""
    outs = []
    for (h, w) in sizes:
        ys, xs = src_index(h, H), src_index(w, W)
        n = 8 if masks is None else masks.shape[-1]
        ty = tap_matrix(axis_ix(boxes[:, 1], boxes[:, 3], H, n, ys), n)          # (O, h, n)
        tx = tap_matrix(axis_ix(boxes[:, 0], boxes[:, 2], W, n, xs), n)          # (O, w, n)
        if masks is None:
            outs.append(torch.einsum("os,oy,ox->syx", vecs, ty.sum(-1), tx.sum(-1)))
        else:
            wgt = torch.einsum("oym,omn,oxn->oyx", ty, masks.to(vecs.dtype), tx)
            outs.append(torch.einsum("os,oyx->syx", vecs, wgt))
    return outs


def paint_ref64(vecs, boxes, masks, H, W, sizes, detail=None):
    """masks_to_layout(test_mode=True): ascending mass = sum(vec) * sum(sampled mask) at full resolution; a pixel goes to
    the first object in that order whose sampled mask is > 0.5 and gets vec * sample."""
    M = masks.shape[-1]
    mk = masks.to(vecs.dtype)

    def weight(h, w):
        ty = tap_matrix(axis_ix(boxes[:, 1], boxes[:, 3], H, M, src_index(h, H)), M)
        tx = tap_matrix(axis_ix(boxes[:, 0], boxes[:, 2], W, M, src_index(w, W)), M)
        return torch.einsum("oym,omn,oxn->oyx", ty, mk, tx)

    mass = vecs.sum(1) * weight(H, W).sum((1, 2))
    order = sorted(range(vecs.shape[0]), key=lambda i: float(mass[i]))
    outs = []
    for (h, w) in sizes:
        wl = weight(h, w)
        out = torch.zeros(vecs.shape[1], h, w, dtype=vecs.dtype)
        free = torch.ones(h, w, dtype=torch.bool)
        for j in order:
            claim = free & (wl[j] > 0.5)
            out = out + vecs[j].view(-1, 1, 1) * (wl[j] * claim.to(vecs.dtype)).unsqueeze(0)
            free = free & ~claim
        outs.append(out)
        if detail is not None:
            detail.setdefault("samples", []).append(wl)
    if detail is not None:
        detail["mass"] = mass
    return outs


def crop_grid(boxes, HH, n_px):
    """(N, HH) un-normalised sample coordinates of a crop axis: crop_bbox's tensor_linspace between the box corners in
    [-1, 1] (bilinear.py:83-94), then align_corners=False (the order of csrc/crop.hip:35-40).  boxes: (N, 2) lo, size."""
    up = torch.linspace(0, 1, steps=HH, dtype=boxes.dtype).view(1, HH)
    down = torch.linspace(1, 0, steps=HH, dtype=boxes.dtype).view(1, HH)
    b0, b1 = 2 * boxes[:, 0:1] - 1, 2 * (boxes[:, 0:1] + boxes[:, 1:2]) - 1
    g = down * b0 + up * b1
    return ((g + 1) * n_px - 1) / 2


def crop_ref64(img, boxes, img_idx, HH):
    """(N, C, HH, HH): out[n, c] = Ty[n] img[idx[n], c] Tx[n]^T with the bilinear tap matrices of the crop's grid."""
    B, C, H, W = img.shape
    tx = tap_matrix(crop_grid(boxes[:, [0, 2]], HH, W), W)                       # (N, HH, W)
    ty = tap_matrix(crop_grid(boxes[:, [1, 3]], HH, H), H)                       # (N, HH, H)
    return torch.einsum("nyh,nchw,nxw->ncyx", ty, img[img_idx], tx)


# --- the same contracts through the oracle (pinned to the reference by tests/golden) and through F.grid_sample
def layout_oracle(vecs, boxes, masks, H, W, sizes):
    import oracle
    full = (oracle.boxes_to_layout(vecs, boxes, H, W) if masks is None else oracle.masks_to_layout(vecs, boxes, masks, H, W))[0]
    return [full[:, src_index(h, H)][:, :, src_index(w, W)] for (h, w) in sizes]


def paint_oracle(vecs, boxes, masks, H, W, sizes):
    import oracle
    if vecs.shape[0] == 0:                           # (the oracle's test mode needs an object to reshape; nothing is painted)
        return [torch.zeros(vecs.shape[1], h, w, dtype=vecs.dtype) for (h, w) in sizes]
    full = oracle.masks_to_layout(vecs, boxes, masks, H, W, test_mode=True)[0]
    return [full[:, src_index(h, H)][:, :, src_index(w, W)] for (h, w) in sizes]


def _layout_grid(boxes, H, W):
    """_boxes_to_grid (layout.py:80-112): (O, H, W, 2)."""
    O = boxes.shape[0]
    x0, y0, ww, hh = (boxes[:, i].view(O, 1, 1) for i in range(4))
    X = (torch.linspace(0, 1, steps=W, dtype=boxes.dtype).view(1, 1, W) - x0) / ww
    Y = (torch.linspace(0, 1, steps=H, dtype=boxes.dtype).view(1, H, 1) - y0) / hh
    return torch.stack([X.expand(O, H, W), Y.expand(O, H, W)], dim=3).mul(2).sub(1)


def layout_grid_sample(vecs, boxes, masks, H, W, sizes):
    """grid_sample is linear in its input, so sampling the constant image vec[o] is vec[o] x the sample of ones: the
    (O, S, H, W) tensor of the reference is never built."""
    O = vecs.shape[0]
    src = torch.ones(O, 1, 8, 8, dtype=vecs.dtype) if masks is None else masks.to(vecs.dtype).unsqueeze(1)
    if O == 0:
        return [torch.zeros(vecs.shape[1], h, w, dtype=vecs.dtype) for (h, w) in sizes]
    smp = F.grid_sample(src, _layout_grid(boxes, H, W), mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    full = torch.einsum("os,oyx->syx", vecs, smp)
    return [full[:, src_index(h, H)][:, :, src_index(w, W)] for (h, w) in sizes]


def crop_grid_sample(img, boxes, img_idx, HH):
    """crop_bbox_batch_cudnn + crop_bbox (bilinear.py:44-94) as oracle.crop_objects evaluates them, in img's precision."""
    N = boxes.shape[0]
    if N == 0:
        return torch.zeros(0, img.shape[1], HH, HH, dtype=img.dtype)
    pts = 2 * torch.stack([boxes[:, 0], boxes[:, 1], boxes[:, 0] + boxes[:, 2], boxes[:, 1] + boxes[:, 3]], dim=1) - 1
    up = torch.linspace(0, 1, steps=HH, dtype=img.dtype).view(1, HH)
    down = torch.linspace(1, 0, steps=HH, dtype=img.dtype).view(1, HH)
    X = down * pts[:, 0:1] + up * pts[:, 2:3]
    Y = down * pts[:, 1:2] + up * pts[:, 3:4]
    grid = torch.stack([X.view(N, 1, HH).expand(N, HH, HH), Y.view(N, HH, 1).expand(N, HH, HH)], dim=3)
    return F.grid_sample(img[img_idx], grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def crop_oracle(img, boxes, img_idx, HH):
    """oracle.crop_objects (pinned to the reference by tests/golden) on crops in any order: the crops are grouped by image
    into the (B, O) arrays it takes, with an `objs` column that marks the real ones, and its (image, object) output order
    is undone.  Its linspace is float32 whatever `img` is, so this is the float32 oracle only."""
    import oracle
    N, B = boxes.shape[0], img.shape[0]
    if N == 0:
        return torch.zeros(0, img.shape[1], HH, HH, dtype=img.dtype)
    perm = torch.argsort(img_idx, stable=True)
    bi = img_idx[perm]
    counts = torch.bincount(bi, minlength=B)
    ji = torch.arange(N) - (torch.cumsum(counts, 0) - counts)[bi]
    O = int(counts.max())
    padded = torch.zeros(B, O, 4, dtype=boxes.dtype).index_put((bi, ji), boxes[perm])
    objs = torch.zeros(B, O, 1, dtype=torch.int64).index_put((bi, ji), torch.ones(N, 1, dtype=torch.int64))
    out, _ = oracle.crop_objects(img, objs, padded, {"object_name_to_idx": {"__image__": -1}}, HH)
    return out[torch.argsort(perm)]


def paint_grid_sample(vecs, boxes, masks, H, W, sizes):
    """test_mode with the mask samples taken by F.grid_sample and the compositing written a third way: every pixel takes
    the claimant (sample > 0.5) of lowest mass rank."""
    O = vecs.shape[0]
    if O == 0:
        return [torch.zeros(vecs.shape[1], h, w, dtype=vecs.dtype) for (h, w) in sizes]
    smp = F.grid_sample(masks.to(vecs.dtype).unsqueeze(1), _layout_grid(boxes, H, W), mode="bilinear", padding_mode="zeros",
                        align_corners=False)[:, 0]                                          # (O, H, W)
    mass = (vecs.view(O, -1, 1, 1) * smp.unsqueeze(1)).sum((1, 2, 3))
    rank = torch.argsort(torch.argsort(mass, stable=True))                                  # rank[o]: position in the order
    key = torch.where(smp > 0.5, rank.view(O, 1, 1).expand_as(smp), torch.full_like(rank.view(O, 1, 1).expand_as(smp), O))
    first = key.min(0)
    owner = torch.where(first.values < O, first.indices, torch.zeros_like(first.indices))
    full = vecs[owner].permute(2, 0, 1) * (smp.gather(0, owner.unsqueeze(0))[0] * (first.values < O).to(vecs.dtype)).unsqueeze(0)
    return [full[:, src_index(h, H)][:, :, src_index(w, W)] for (h, w) in sizes]


# REF64: this file's restatement.  ORACLE: the oracle's functions, pinned by tests/golden (crops: float32 only, see
# crop_oracle).  GRID_SAMPLE: torch's operator on the reference's own sampling grids, in any precision.
REF64 = dict(layout=layout_ref64, paint=paint_ref64, crop=crop_ref64)
ORACLE = dict(layout=layout_oracle, paint=paint_oracle, crop=crop_oracle)
GRID_SAMPLE = dict(layout=layout_grid_sample, paint=paint_grid_sample, crop=crop_grid_sample)


def _leaf(t, dtype):
    return t.detach().clone().to(dtype)


def evaluate(c, d, fns=REF64, dtype=torch.float64):
    """{tensor name: tensor or None}: the row's outputs ("out0", "out1", ... — NCHW) and the gradients of
    sum_levels <out, dout> with respect to what the row needs ("dvecs", "dboxes", "dmasks", "dimg"), through autograd."""
    need = c["need"]
    if c["family"] == "crop":
        img = _leaf(d["img"], dtype).requires_grad_("img" in need)
        boxes = _leaf(d["boxes"], dtype).requires_grad_("boxes" in need)
        C = c["C"]
        out = fns["crop"](img, boxes, d["img_idx"], c["HH"])
        res = dict(out0=F.pad(out.detach(), (0, 0, 0, 0, 0, d["dout"].shape[1] - C)), dimg=None, dboxes=None)
        if need:
            if out.requires_grad:                    # (no crop at all: nothing depends on the leaves)
                (out * d["dout"][:, :C].to(dtype)).sum().backward()
            res["dimg"], res["dboxes"] = img.grad, boxes.grad
            if res["dimg"] is None and "img" in need:
                res["dimg"] = torch.zeros_like(img)
            if res["dboxes"] is None and "boxes" in need:
                res["dboxes"] = torch.zeros_like(boxes)
        return res
    B, S, H, W = c["B"], c["S"], c["H"], c["W"]
    vecs = _leaf(d["vecs"], dtype).requires_grad_("vecs" in need)
    boxes = _leaf(d["boxes"], dtype).requires_grad_("boxes" in need)
    masks = d["masks"]
    if masks is not None and masks.is_floating_point():
        masks = _leaf(masks, dtype).requires_grad_("masks" in need)
    img = _leaf(d["img"], dtype).requires_grad_("img" in need) if c["entry"] == "disc_input" else None
    fn = fns["paint" if c["entry"] == "layout_paint" else "layout"]
    levels = [[] for _ in c["sizes"]]
    for b in range(B):
        v = d["valid"][b].nonzero().flatten()
        outs = fn(vecs[b][v], boxes[b][v], None if masks is None else masks[b][v], H, W, c["sizes"])
        for lv, o in zip(levels, outs):
            lv.append(o)
    outs = [torch.stack(lv) for lv in levels]
    if img is not None:
        Ct = d["douts"][0].shape[1]
        outs = [torch.cat([outs[0], img, torch.zeros(B, Ct - S - 3, H, H, dtype=dtype)], 1)]
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    res.update(dvecs=None, dboxes=None, dmasks=None, dimg=None)
    if need:
        loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, d["douts"]))
        if loss.requires_grad:                       # (no object at all: nothing depends on the leaves)
            loss.backward()
        for name, leaf in (("dvecs", vecs), ("dboxes", boxes), ("dmasks", masks), ("dimg", img)):
            if name[1:] in need:
                res[name] = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    if c["entry"] != "disc_input":
        del res["dimg"]
    return res


def geom_ref64(c, d):
    return evaluate(c, d, REF64, torch.float64)


# ------------------------------------------------------------------------------------------------- discontinuities
def _floor_mismatch(ix64, ix32, n_src):
    """Samples that can contribute (a tap inside the source, or the derivative's support, in either precision) whose
    float32 coordinate lies in another bilinear cell than the float64 one."""
    ix32 = ix32.to(torch.float64)
    near = ((ix64 >= -2) & (ix64 <= n_src + 1)) | ((ix32 >= -2) & (ix32 <= n_src + 1))
    return int((near & (torch.floor(ix64) != torch.floor(ix32))).sum())


def floor_mismatches(c, d):
    """Condition (a): 0 for a row whose every contributing (object, pixel, axis) has the same floor() in float32, evaluated
    in ATen's order, as in float64."""
    bad = 0
    if c["family"] == "crop":
        for cols, n_px in (([0, 2], c["W"]), ([1, 3], c["H"])):
            bx = d["boxes"][:, cols]
            bad += _floor_mismatch(crop_grid(bx, c["HH"], n_px), crop_grid(bx.float(), c["HH"], n_px), n_px)
        return bad
    n = c["masks"][1] if c["masks"] else 8
    for b in range(c["B"]):
        bx = d["boxes"][b][d["valid"][b]]
        for lo, size, n_px in ((0, 2, c["W"]), (1, 3, c["H"])):
            bad += _floor_mismatch(axis_ix(bx[:, lo], bx[:, size], n_px, n), axis_ix(bx[:, lo].float(), bx[:, size].float(), n_px, n), n)
    return bad


def paint_margins(c, d):
    """Conditions (b) and (c) of a paint row: (smallest relative gap between two valid objects' masses in one image,
    smallest distance of a sampled mask value from 0.5 over every level)."""
    gap, thr = float("inf"), float("inf")
    for b in range(c["B"]):
        v = d["valid"][b].nonzero().flatten()
        if len(v) == 0:
            continue
        detail = {}
        paint_ref64(d["vecs"][b][v], d["boxes"][b][v], d["masks"][b][v], c["H"], c["W"], c["sizes"], detail)
        m = detail["mass"]
        for i in range(len(m)):
            for j in range(i):
                gap = min(gap, float((m[i] - m[j]).abs() / torch.maximum(m[i].abs(), m[j].abs()).clamp_min(1e-300)))
        for s in detail["samples"]:
            thr = min(thr, float((s - 0.5).abs().min()))
    return gap, thr


# ------------------------------------------------------------------------------------------------- the culls, restated
def tile_survivors(c, d, level, rows_per_block):
    """Largest number of objects one block keeps after its cull (csrc/layout.hip:188-211 forward, :471-483 tiled backward):
    valid, a non-zero row weight on one of the block's rows, and an x support that meets the block's pixel chunk with one
    pixel of slack."""
    (h, w), H, W = c["sizes"][level], c["H"], c["W"]
    r = level_rules(c)[level]
    n = c["masks"][1] if c["masks"] else 8
    ys, xs = src_index(h, H), src_index(w, W)
    t = torch.linspace(0, 1, steps=W, dtype=torch.float64)
    step = 1.0 / (W - 1) if W > 1 else 1.0
    best = 0
    for b in range(c["B"]):
        v = d["valid"][b]
        bx = d["boxes"][b]
        rowsum = tap_matrix(axis_ix(bx[:, 1], bx[:, 3], H, n, ys), n).sum(-1) != 0           # (O, h)
        e0, e1 = bx[:, 0] - bx[:, 2] / (2 * n), bx[:, 0] + bx[:, 2] * (1 + 1 / (2 * n))
        lo, hi = torch.minimum(e0, e1), torch.maximum(e0, e1)
        for y0 in range(0, h, rows_per_block):
            ya = rowsum[:, y0:y0 + rows_per_block].any(1)
            for x0 in range(0, w, r["pxc"]):
                x1 = min(x0 + r["pxc"], w) - 1
                keep = v & ya & ~((t[xs[x1]] + step < lo) | (t[xs[x0]] - step > hi))
                best = max(best, int(keep.sum()))
    return best


def crop_tile_candidates(c, d):
    """Largest number of crops one 16 x 16 tile of k_crop_bwd lists (the footprint test of csrc/crop.hip:115-120)."""
    H, W, bx = c["H"], c["W"], d["boxes"]
    if c["N"] == 0:
        return 0
    fx0, fx1 = bx[:, 0] * W - 0.5, (bx[:, 0] + bx[:, 2]) * W - 0.5
    fy0, fy1 = bx[:, 1] * H - 0.5, (bx[:, 1] + bx[:, 3]) * H - 0.5
    best = 0
    for b in range(c["B"]):
        for ty0 in range(0, H, CROP_TILE):
            for tx0 in range(0, W, CROP_TILE):
                take = ((d["img_idx"] == b) & (torch.minimum(fx0, fx1) - 2 <= tx0 + 15) & (torch.maximum(fx0, fx1) + 2 >= tx0) &
                        (torch.minimum(fy0, fy1) - 2 <= ty0 + 15) & (torch.maximum(fy0, fy1) + 2 >= ty0))
                best = max(best, int(take.sum()))
    return best


def crop_slopes(c, d):
    """(N, 2): the grid's slope in source pixels per crop pixel along x and y (csrc/crop.hip:149)."""
    den = max(c["HH"] - 1, 1)
    return torch.stack([d["boxes"][:, 2] * c["W"] / den, d["boxes"][:, 3] * c["H"] / den], 1)
