"""Inception-v3, forward only, on the library's kernels: the network behind FID and the Inception score.

Two variants of ONE architecture (torchvision's public `inception_v3`, restated here because torchvision cannot be imported
where this is built):

* ``variant="torchvision"`` — `inception_v3(transform_input=False)` as the reference's Inception score uses it
  (evaluation/inception.py:16): logits from `fc` 2048 -> 1000.
* ``variant="fid"`` — the reference's `fid_inception_v3` (evaluation/fid/inception.py:166-310): `fc` 2048 -> 1008, the average
  pools of the A, C and first E blocks leave the padding out of their divisor, `Mixed_7c` pools with a max; outputs by
  `dims` (BLOCK_INDEX_BY_DIM, :24-29), each the spatial mean of the stated layer's output.

`state_dict()` has torchvision's keys, so `inception_v3_google-*.pth` and `pt_inception-2015-12-05-*.pth` load strictly; the
only keys ignored are `AuxLogits.*` and `*.num_batches_tracked`.  LOADING THE REAL FILES AND THE NUMBERS THEY GIVE ARE
UNCHECKED HERE: neither file is available where this is built and tested; every test runs the seeded stand-in
(`weights="random"`), which is for tests and throughput only.

How it runs: BatchNorm (eps 1e-3) is folded into weight and bias once per load, on the host, in fp64; ReLU rides in the
convolution epilogue (ACT_LEAKY, slope 0); square layers with an output of their own go through `ops.conv2d` under no_grad
(`plan_conv` picks the kernel); the rectangular layers and every layer that ends a branch go through `ops.conv2d_forward`,
which writes the branch straight into its channel slice of the block's output — no `torch.cat` copy.
"""
import collections
import os

import torch
import torch.nn as nn

from . import ops
from .ops import ACT_LEAKY, POOL_AVG9, POOL_AVG_INSIDE, POOL_MAX

BN_EPS = 1e-3
WEIGHT_FILES = {"torchvision": "inception_v3_google-*.pth", "fid": "pt_inception-2015-12-05-*.pth"}
WEIGHT_ENV = {"torchvision": "CSG_INCEPTION_WEIGHTS", "fid": "CSG_FID_INCEPTION_WEIGHTS"}
DIMS = (64, 192, 768, 2048)          # evaluation/fid/inception.py:24-29

Layer = collections.namedtuple("Layer", "name cin cout kh kw stride ph pw")


def _sq(name, cin, cout, k, stride=1, pad=0):
    return Layer(name, cin, cout, k, k, stride, pad, pad)


def _rect(name, cin, cout, kh, kw):
    return Layer(name, cin, cout, kh, kw, 1, kh // 2, kw // 2)


def _block_a(p, cin, pf):
    return [_sq(p + "branch1x1", cin, 64, 1), _sq(p + "branch5x5_1", cin, 48, 1), _sq(p + "branch5x5_2", 48, 64, 5, 1, 2),
            _sq(p + "branch3x3dbl_1", cin, 64, 1), _sq(p + "branch3x3dbl_2", 64, 96, 3, 1, 1),
            _sq(p + "branch3x3dbl_3", 96, 96, 3, 1, 1), _sq(p + "branch_pool", cin, pf, 1)]


def _block_b(p, cin):
    return [_sq(p + "branch3x3", cin, 384, 3, 2), _sq(p + "branch3x3dbl_1", cin, 64, 1),
            _sq(p + "branch3x3dbl_2", 64, 96, 3, 1, 1), _sq(p + "branch3x3dbl_3", 96, 96, 3, 2)]


def _block_c(p, cin, c7):
    return [_sq(p + "branch1x1", cin, 192, 1), _sq(p + "branch7x7_1", cin, c7, 1), _rect(p + "branch7x7_2", c7, c7, 1, 7),
            _rect(p + "branch7x7_3", c7, 192, 7, 1), _sq(p + "branch7x7dbl_1", cin, c7, 1),
            _rect(p + "branch7x7dbl_2", c7, c7, 7, 1), _rect(p + "branch7x7dbl_3", c7, c7, 1, 7),
            _rect(p + "branch7x7dbl_4", c7, c7, 7, 1), _rect(p + "branch7x7dbl_5", c7, 192, 1, 7),
            _sq(p + "branch_pool", cin, 192, 1)]


def _block_d(p, cin):
    return [_sq(p + "branch3x3_1", cin, 192, 1), _sq(p + "branch3x3_2", 192, 320, 3, 2), _sq(p + "branch7x7x3_1", cin, 192, 1),
            _rect(p + "branch7x7x3_2", 192, 192, 1, 7), _rect(p + "branch7x7x3_3", 192, 192, 7, 1),
            _sq(p + "branch7x7x3_4", 192, 192, 3, 2)]


def _block_e(p, cin):
    return [_sq(p + "branch1x1", cin, 320, 1), _sq(p + "branch3x3_1", cin, 384, 1), _rect(p + "branch3x3_2a", 384, 384, 1, 3),
            _rect(p + "branch3x3_2b", 384, 384, 3, 1), _sq(p + "branch3x3dbl_1", cin, 448, 1),
            _sq(p + "branch3x3dbl_2", 448, 384, 3, 1, 1), _rect(p + "branch3x3dbl_3a", 384, 384, 1, 3),
            _rect(p + "branch3x3dbl_3b", 384, 384, 3, 1), _sq(p + "branch_pool", cin, 192, 1)]


def layer_table():
    """The 94 convolutions in torchvision's order: Layer(name, cin, cout, kh, kw, stride, pad_h, pad_w)."""
    t = [_sq("Conv2d_1a_3x3", 3, 32, 3, 2), _sq("Conv2d_2a_3x3", 32, 32, 3), _sq("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
         _sq("Conv2d_3b_1x1", 64, 80, 1), _sq("Conv2d_4a_3x3", 80, 192, 3)]
    t += _block_a("Mixed_5b.", 192, 32) + _block_a("Mixed_5c.", 256, 64) + _block_a("Mixed_5d.", 288, 64)
    t += _block_b("Mixed_6a.", 288)
    for name, c7 in (("Mixed_6b.", 128), ("Mixed_6c.", 160), ("Mixed_6d.", 160), ("Mixed_6e.", 192)):
        t += _block_c(name, 768, c7)
    t += _block_d("Mixed_7a.", 768) + _block_e("Mixed_7b.", 1280) + _block_e("Mixed_7c.", 2048)
    return t


BLOCKS = (("Mixed_5b", "A"), ("Mixed_5c", "A"), ("Mixed_5d", "A"), ("Mixed_6a", "B"), ("Mixed_6b", "C"), ("Mixed_6c", "C"),
          ("Mixed_6d", "C"), ("Mixed_6e", "C"), ("Mixed_7a", "D"), ("Mixed_7b", "E"), ("Mixed_7c", "E"))


def state_dict_keys(variant):
    """Every key of `state_dict()`: 5 per convolution (conv.weight and the BatchNorm's four) + fc.weight, fc.bias."""
    keys = []
    for L in layer_table():
        keys += [L.name + ".conv.weight"] + [L.name + ".bn." + s for s in ("weight", "bias", "running_mean", "running_var")]
    return keys + ["fc.weight", "fc.bias"]


def random_state_dict(variant, seed=0):
    """The seeded STAND-IN for a weights file (tests and throughput only — its features mean nothing): He-scaled normal
    convolution weights and BatchNorm statistics near the identity, so that activations keep their scale through 94 layers."""
    g = torch.Generator().manual_seed(1000 + seed + (0 if variant == "torchvision" else 1))
    sd = collections.OrderedDict()
    for L in layer_table():
        fan = L.cin * L.kh * L.kw
        sd[L.name + ".conv.weight"] = torch.randn(L.cout, L.cin, L.kh, L.kw, generator=g) * (2.0 / fan) ** 0.5
        sd[L.name + ".bn.weight"] = 0.75 + 0.5 * torch.rand(L.cout, generator=g)
        sd[L.name + ".bn.bias"] = 0.2 * torch.randn(L.cout, generator=g)
        sd[L.name + ".bn.running_mean"] = 0.2 * torch.randn(L.cout, generator=g)
        sd[L.name + ".bn.running_var"] = 0.5 + torch.rand(L.cout, generator=g)
    rows = 1000 if variant == "torchvision" else 1008
    sd["fc.weight"] = torch.randn(rows, 2048, generator=g) * (1.0 / 2048) ** 0.5
    sd["fc.bias"] = 0.1 * torch.randn(rows, generator=g)
    return sd


def fold_batchnorm(weight, gamma, beta, mean, var, eps=BN_EPS):
    """(w', b') of conv -> BatchNorm(eval) as one convolution with bias, computed in fp64: w' = w * gamma / sqrt(var + eps)
    per output channel, b' = beta - mean * gamma / sqrt(var + eps).  Returns fp64 tensors."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return weight.double() * s.view(-1, 1, 1, 1), beta.double() - mean.double() * s


class _Bare(nn.Module):
    """A holder of parameters / buffers under torchvision's names (`conv`, `bn`, `fc`); it computes nothing."""


def _basic_conv(L):
    m = _Bare()
    m.conv = _Bare()
    m.conv.weight = nn.Parameter(torch.zeros(L.cout, L.cin, L.kh, L.kw), requires_grad=False)
    m.bn = _Bare()
    m.bn.weight = nn.Parameter(torch.ones(L.cout), requires_grad=False)
    m.bn.bias = nn.Parameter(torch.zeros(L.cout), requires_grad=False)
    m.bn.register_buffer("running_mean", torch.zeros(L.cout))
    m.bn.register_buffer("running_var", torch.ones(L.cout))
    return m


class InceptionV3(nn.Module):
    """InceptionV3(variant, weights): forward only, eval mode only.

    weights: a path to the variant's file (WEIGHT_FILES), a state dict, "random" (the seeded stand-in, `stand_in = True`,
    labelled so in every output built on it), or None: the file named by $CSG_INCEPTION_WEIGHTS ("torchvision") /
    $CSG_FID_INCEPTION_WEIGHTS ("fid"); without one the constructor raises.

    forward(x, dims=None): x logical (B, 3 or 4, H, W) fp32 on the device, already resized and scaled (see `prepare`).
    "torchvision": the (B, 1000) logits.  "fid": the (B, dims) features, dims in DIMS (default 2048); `dims` may be a tuple,
    the result is then a list.  The 1008-row `fc` of the "fid" variant is loaded and kept but, as in the reference, not run."""

    def __init__(self, variant, weights=None):
        super().__init__()
        if variant not in WEIGHT_FILES:
            raise ValueError("InceptionV3: variant must be 'torchvision' or 'fid', got %r" % (variant,))
        self.variant = variant
        self.table = layer_table()
        for L in self.table:
            parent, leaf = self, L.name
            if "." in L.name:
                block, leaf = L.name.split(".")
                if not hasattr(self, block):
                    setattr(self, block, _Bare())
                parent = getattr(self, block)
            setattr(parent, leaf, _basic_conv(L))
        rows = 1000 if variant == "torchvision" else 1008
        self.fc = _Bare()
        self.fc.weight = nn.Parameter(torch.zeros(rows, 2048), requires_grad=False)
        self.fc.bias = nn.Parameter(torch.zeros(rows), requires_grad=False)
        self._folded = None
        self.stand_in = False
        if weights is None:
            weights = os.environ.get(WEIGHT_ENV[variant]) or None
        if weights is None:
            raise RuntimeError(
                "InceptionV3(%r): no weights.  The Inception score needs torchvision's %s, FID needs pytorch-fid's %s; pass "
                "the file (or a state dict) as weights=, or name it in $%s.  weights='random' gives a seeded stand-in for "
                "tests and throughput runs only — its numbers mean nothing."
                % (variant, WEIGHT_FILES["torchvision"], WEIGHT_FILES["fid"], WEIGHT_ENV[variant]))
        if isinstance(weights, str) and weights == "random":
            self.stand_in = True
            self.load_state_dict(random_state_dict(variant))
        elif isinstance(weights, (str, os.PathLike)):
            sd = torch.load(weights, map_location="cpu")
            self.load_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)
        else:
            self.load_state_dict(weights)
        super().train(False)

    # ---- the state dict: torchvision's keys, strict
    def load_state_dict(self, state_dict, strict=True):
        """Strict over torchvision's keys; `AuxLogits.*` and `*.num_batches_tracked` are the only keys ignored."""
        sd = collections.OrderedDict((k, v) for k, v in state_dict.items()
                                     if not k.startswith("AuxLogits.") and not k.endswith(".num_batches_tracked"))
        self._folded = None
        return super().load_state_dict(sd, strict=strict)

    def train(self, mode=True):
        if mode:
            raise RuntimeError("InceptionV3 is eval mode only: BatchNorm is folded into the convolutions at load")
        return super().train(False)

    def _apply(self, fn, *args, **kwargs):
        self._folded = None
        return super()._apply(fn, *args, **kwargs)

    def _fold(self, device):
        """Once per load and device: BatchNorm folded in fp64 on the host; weights [Cout][KH][KW][Cin] (the picture's 3
        input channels zero-padded to 4) and biases in fp32 on the device."""
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        folded = {}
        for L in self.table:
            w, b = fold_batchnorm(sd[L.name + ".conv.weight"], sd[L.name + ".bn.weight"], sd[L.name + ".bn.bias"],
                                  sd[L.name + ".bn.running_mean"], sd[L.name + ".bn.running_var"])
            if L.cin % 4:
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, (-L.cin) % 4))
            folded[L.name] = (w.permute(0, 2, 3, 1).contiguous().float().to(device), b.float().to(device))
        folded["fc"] = (sd["fc.weight"].float().contiguous().to(device), sd["fc.bias"].float().to(device))
        self._folded = (device, folded)

    # ---- the forward
    def _conv(self, L, x, out=None, off=0):
        wp, b = self._folded[1][L.name]
        if out is None and L.kh == L.kw and L.kh * L.kw <= 16:
            # a square layer with an output of its own: the ordinary entry, plan_conv picks the kernel
            return ops.conv2d(x, wp.permute(0, 3, 1, 2), b, L.stride, L.ph, ACT_LEAKY, 0.0)
        return ops.conv2d_forward(x, wp, b, L.kh, L.kw, L.stride, (L.ph, L.pw), ACT_LEAKY, 0.0, out=out, out_off=off)

    def _block(self, name, kind, x):
        Ls = {L.name[len(name) + 1:]: L for L in self.table if L.name.startswith(name + ".")}
        c = self._conv
        B, _, H, W = x.shape
        fid = self.variant == "fid"
        avg = POOL_AVG_INSIDE if fid else POOL_AVG9
        if kind == "A":
            pf = Ls["branch_pool"].cout
            y = ops.empty_nhwc(B, 224 + pf, H, W, x.device)
            c(Ls["branch1x1"], x, y, 0)
            c(Ls["branch5x5_2"], c(Ls["branch5x5_1"], x), y, 64)
            c(Ls["branch3x3dbl_3"], c(Ls["branch3x3dbl_2"], c(Ls["branch3x3dbl_1"], x)), y, 128)
            c(Ls["branch_pool"], ops.pool3(x, avg, 1, 1), y, 224)
        elif kind == "B":
            OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
            y = ops.empty_nhwc(B, 480 + x.shape[1], OH, OW, x.device)
            c(Ls["branch3x3"], x, y, 0)
            c(Ls["branch3x3dbl_3"], c(Ls["branch3x3dbl_2"], c(Ls["branch3x3dbl_1"], x)), y, 384)
            ops.pool3(x, POOL_MAX, 2, 0, out=y, out_off=480)
        elif kind == "C":
            y = ops.empty_nhwc(B, 768, H, W, x.device)
            c(Ls["branch1x1"], x, y, 0)
            c(Ls["branch7x7_3"], c(Ls["branch7x7_2"], c(Ls["branch7x7_1"], x)), y, 192)
            t = c(Ls["branch7x7dbl_1"], x)
            for k in ("branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4"):
                t = c(Ls[k], t)
            c(Ls["branch7x7dbl_5"], t, y, 384)
            c(Ls["branch_pool"], ops.pool3(x, avg, 1, 1), y, 576)
        elif kind == "D":
            OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
            y = ops.empty_nhwc(B, 512 + x.shape[1], OH, OW, x.device)
            c(Ls["branch3x3_2"], c(Ls["branch3x3_1"], x), y, 0)
            t = c(Ls["branch7x7x3_1"], x)
            for k in ("branch7x7x3_2", "branch7x7x3_3"):
                t = c(Ls[k], t)
            c(Ls["branch7x7x3_4"], t, y, 320)
            ops.pool3(x, POOL_MAX, 2, 0, out=y, out_off=512)
        elif kind == "E":
            y = ops.empty_nhwc(B, 2048, H, W, x.device)
            c(Ls["branch1x1"], x, y, 0)
            t = c(Ls["branch3x3_1"], x)
            c(Ls["branch3x3_2a"], t, y, 320)
            c(Ls["branch3x3_2b"], t, y, 704)
            t = c(Ls["branch3x3dbl_2"], c(Ls["branch3x3dbl_1"], x))
            c(Ls["branch3x3dbl_3a"], t, y, 1088)
            c(Ls["branch3x3dbl_3b"], t, y, 1472)
            pool = POOL_MAX if (fid and name == "Mixed_7c") else avg
            c(Ls["branch_pool"], ops.pool3(x, pool, 1, 1), y, 1856)
        else:
            raise ValueError(kind)
        return y

    def run_block(self, name, x):
        """One Mixed_* block on its own (tests): x logical (B, Cin, H, W) on the device."""
        self._refuse_gradients(x)
        with torch.no_grad():
            x = self._ready(x)
            return self._block(name, dict(BLOCKS)[name], x)

    @staticmethod
    def _refuse_gradients(x):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("InceptionV3 is forward only: gradients are refused (the network is a frozen metric); detach "
                               "the images or call it under torch.no_grad()")

    def _ready(self, x):
        if not x.is_cuda:
            raise RuntimeError("InceptionV3 needs HIP (cuda) tensors; got a %s tensor — there is no CPU path" % x.device)
        if self._folded is None or self._folded[0] != x.device:
            self._fold(x.device)
        return ops.nhwc(x.detach())

    def forward(self, x, dims=None):
        if self.variant == "torchvision":
            if dims is not None:
                raise ValueError("InceptionV3('torchvision') returns logits; dims= belongs to the 'fid' variant")
            want = ()
        else:
            want = (2048,) if dims is None else ((dims,) if isinstance(dims, int) else tuple(dims))
            if not want or any(d not in DIMS for d in want):
                raise ValueError("InceptionV3('fid'): dims must be among %s, got %r" % (DIMS, dims))
        self._refuse_gradients(x)
        with torch.no_grad():
            x = self._ready(x)
            if x.shape[1] == 3:
                x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, 1))
                x = ops.nhwc(x)
            elif x.shape[1] != 4:
                raise RuntimeError("InceptionV3: images must have 3 channels (or 4, the last zero), got %d" % x.shape[1])
            by = {L.name: L for L in self.table}
            feats = {}
            last = max(want) if want else 2048
            x = self._conv(by["Conv2d_1a_3x3"], x)
            x = self._conv(by["Conv2d_2a_3x3"], x)
            x = self._conv(by["Conv2d_2b_3x3"], x)
            x = ops.pool3(x, POOL_MAX, 2, 0)
            if 64 in want:
                feats[64] = ops.spatial_mean(x)
            if last >= 192:
                x = self._conv(by["Conv2d_3b_1x1"], x)
                x = self._conv(by["Conv2d_4a_3x3"], x)
                x = ops.pool3(x, POOL_MAX, 2, 0)
                if 192 in want:
                    feats[192] = ops.spatial_mean(x)
            if last >= 768:
                for name, kind in BLOCKS[:8]:
                    x = self._block(name, kind, x)
                if 768 in want:
                    feats[768] = ops.spatial_mean(x)
            if last >= 2048:
                for name, kind in BLOCKS[8:]:
                    x = self._block(name, kind, x)
                pooled = ops.spatial_mean(x)
                if 2048 in want:
                    feats[2048] = pooled
            if self.variant == "torchvision":
                fw, fb = self._folded[1]["fc"]
                return ops.linear(pooled, fw, fb)
            out = [feats[d] for d in want]
            return out[0] if (dims is None or isinstance(dims, int)) else out


def prepare(images, variant, size=(299, 299), channel_order="rgb"):
    """The input stage in front of the network, one launch: bilinear resize (align_corners=False, no antialiasing) to `size`
    and the variant's affine.  "fid": 2x - 1 on [0, 1] values (evaluation/fid/inception.py:146-153) — uint8 pictures
    (B,H,W,3) are divided by 255 first (fid_score.py:115); "torchvision": identity on the generator's output, as
    evaluation/inception.py:23-27 feeds it.  channel_order="bgr" reverses the channels (what a cv2.imread reader hands on).
    size=None: no resize (the map keeps its size; still one pass for the affine and the 4-channel padding)."""
    if channel_order not in ("rgb", "bgr"):
        raise ValueError("channel_order must be 'rgb' or 'bgr'")
    if images.dtype == torch.uint8:
        H, W = images.shape[1], images.shape[2]
    else:
        H, W = images.shape[2], images.shape[3]
    a, b = (2.0, -1.0) if variant == "fid" else (1.0, 0.0)
    return ops.resize_bilinear(images, (H, W) if size is None else size, a, b, reverse=channel_order == "bgr")
