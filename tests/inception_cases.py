"""Inception-v3 restated in plain torch.nn.functional with UNFOLDED BatchNorm, for the CPU in any dtype (float64 is the
reference of tests/test_gpu_inception.py), seeded weights, and the case tables of the quality tests.  Written from
torchvision's public architecture and the reference's evaluation/fid/inception.py:193-310, independently of
canonicalsg2im_amd/inception.py: no table or helper of the package is used here."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3
DIMS = (64, 192, 768, 2048)


# ---------------------------------------------------------------------------------------------- the 94 convolutions
def _names_a(p):
    return [p + n for n in ("branch1x1", "branch5x5_1", "branch5x5_2", "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3",
                            "branch_pool")]


def conv_shapes():
    """{name: (cout, cin, kh, kw)} of every BasicConv2d, in torchvision's order."""
    s = {"Conv2d_1a_3x3": (32, 3, 3, 3), "Conv2d_2a_3x3": (32, 32, 3, 3), "Conv2d_2b_3x3": (64, 32, 3, 3),
         "Conv2d_3b_1x1": (80, 64, 1, 1), "Conv2d_4a_3x3": (192, 80, 3, 3)}
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        p = blk + "."
        s.update({p + "branch1x1": (64, cin, 1, 1), p + "branch5x5_1": (48, cin, 1, 1), p + "branch5x5_2": (64, 48, 5, 5),
                  p + "branch3x3dbl_1": (64, cin, 1, 1), p + "branch3x3dbl_2": (96, 64, 3, 3),
                  p + "branch3x3dbl_3": (96, 96, 3, 3), p + "branch_pool": (pf, cin, 1, 1)})
    p = "Mixed_6a."
    s.update({p + "branch3x3": (384, 288, 3, 3), p + "branch3x3dbl_1": (64, 288, 1, 1), p + "branch3x3dbl_2": (96, 64, 3, 3),
              p + "branch3x3dbl_3": (96, 96, 3, 3)})
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        p = blk + "."
        s.update({p + "branch1x1": (192, 768, 1, 1), p + "branch7x7_1": (c7, 768, 1, 1), p + "branch7x7_2": (c7, c7, 1, 7),
                  p + "branch7x7_3": (192, c7, 7, 1), p + "branch7x7dbl_1": (c7, 768, 1, 1),
                  p + "branch7x7dbl_2": (c7, c7, 7, 1), p + "branch7x7dbl_3": (c7, c7, 1, 7),
                  p + "branch7x7dbl_4": (c7, c7, 7, 1), p + "branch7x7dbl_5": (192, c7, 1, 7),
                  p + "branch_pool": (192, 768, 1, 1)})
    p = "Mixed_7a."
    s.update({p + "branch3x3_1": (192, 768, 1, 1), p + "branch3x3_2": (320, 192, 3, 3), p + "branch7x7x3_1": (192, 768, 1, 1),
              p + "branch7x7x3_2": (192, 192, 1, 7), p + "branch7x7x3_3": (192, 192, 7, 1),
              p + "branch7x7x3_4": (192, 192, 3, 3)})
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        p = blk + "."
        s.update({p + "branch1x1": (320, cin, 1, 1), p + "branch3x3_1": (384, cin, 1, 1), p + "branch3x3_2a": (384, 384, 1, 3),
                  p + "branch3x3_2b": (384, 384, 3, 1), p + "branch3x3dbl_1": (448, cin, 1, 1),
                  p + "branch3x3dbl_2": (384, 448, 3, 3), p + "branch3x3dbl_3a": (384, 384, 1, 3),
                  p + "branch3x3dbl_3b": (384, 384, 3, 1), p + "branch_pool": (192, cin, 1, 1)})
    return s


def fc_rows(variant):
    return 1000 if variant == "torchvision" else 1008


def seeded_state_dict(variant, seed=0):
    """A state dict with torchvision's keys: He-scaled weights, BatchNorm statistics away from the identity (so that a slip
    in the folding shows), float32."""
    g = torch.Generator().manual_seed(77 + seed + (0 if variant == "torchvision" else 1))
    sd = {}
    for name, (co, ci, kh, kw) in conv_shapes().items():
        sd[name + ".conv.weight"] = torch.randn(co, ci, kh, kw, generator=g) * (2.0 / (ci * kh * kw)) ** 0.5
        sd[name + ".bn.weight"] = 0.6 + 0.8 * torch.rand(co, generator=g)
        sd[name + ".bn.bias"] = 0.3 * torch.randn(co, generator=g)
        sd[name + ".bn.running_mean"] = 0.3 * torch.randn(co, generator=g)
        sd[name + ".bn.running_var"] = 0.4 + 1.2 * torch.rand(co, generator=g)
    sd["fc.weight"] = torch.randn(fc_rows(variant), 2048, generator=g) * (1.0 / 2048) ** 0.5
    sd["fc.bias"] = 0.1 * torch.randn(fc_rows(variant), generator=g)
    return sd


# ---------------------------------------------------------------------------------------------- the restatement
class Net:
    """net = Net(state_dict, variant, dtype); net(x) / net.block(name, x) on CPU tensors of that dtype."""

    def __init__(self, sd, variant, dtype=torch.float64):
        self.sd = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
        self.variant, self.dtype = variant, dtype

    def bc(self, name, x, stride=1, padding=0):
        sd = self.sd
        y = F.conv2d(x, sd[name + ".conv.weight"], None, stride, padding)
        y = F.batch_norm(y, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"],
                         sd[name + ".bn.bias"], False, 0.0, EPS)
        return F.relu(y)

    def avg(self, x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=self.variant != "fid")

    def block_a(self, p, x):
        b1 = self.bc(p + "branch1x1", x)
        b5 = self.bc(p + "branch5x5_2", self.bc(p + "branch5x5_1", x), padding=2)
        b3 = self.bc(p + "branch3x3dbl_1", x)
        b3 = self.bc(p + "branch3x3dbl_3", self.bc(p + "branch3x3dbl_2", b3, padding=1), padding=1)
        bp = self.bc(p + "branch_pool", self.avg(x))
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, p, x):
        b3 = self.bc(p + "branch3x3", x, stride=2)
        bd = self.bc(p + "branch3x3dbl_2", self.bc(p + "branch3x3dbl_1", x), padding=1)
        bd = self.bc(p + "branch3x3dbl_3", bd, stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def block_c(self, p, x):
        b1 = self.bc(p + "branch1x1", x)
        b7 = self.bc(p + "branch7x7_1", x)
        b7 = self.bc(p + "branch7x7_2", b7, padding=(0, 3))
        b7 = self.bc(p + "branch7x7_3", b7, padding=(3, 0))
        bd = self.bc(p + "branch7x7dbl_1", x)
        bd = self.bc(p + "branch7x7dbl_2", bd, padding=(3, 0))
        bd = self.bc(p + "branch7x7dbl_3", bd, padding=(0, 3))
        bd = self.bc(p + "branch7x7dbl_4", bd, padding=(3, 0))
        bd = self.bc(p + "branch7x7dbl_5", bd, padding=(0, 3))
        bp = self.bc(p + "branch_pool", self.avg(x))
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, p, x):
        b3 = self.bc(p + "branch3x3_2", self.bc(p + "branch3x3_1", x), stride=2)
        b7 = self.bc(p + "branch7x7x3_1", x)
        b7 = self.bc(p + "branch7x7x3_2", b7, padding=(0, 3))
        b7 = self.bc(p + "branch7x7x3_3", b7, padding=(3, 0))
        b7 = self.bc(p + "branch7x7x3_4", b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def block_e(self, p, x):
        b1 = self.bc(p + "branch1x1", x)
        b3 = self.bc(p + "branch3x3_1", x)
        b3 = torch.cat([self.bc(p + "branch3x3_2a", b3, padding=(0, 1)), self.bc(p + "branch3x3_2b", b3, padding=(1, 0))], 1)
        bd = self.bc(p + "branch3x3dbl_2", self.bc(p + "branch3x3dbl_1", x), padding=1)
        bd = torch.cat([self.bc(p + "branch3x3dbl_3a", bd, padding=(0, 1)), self.bc(p + "branch3x3dbl_3b", bd, padding=(1, 0))], 1)
        if self.variant == "fid" and p == "Mixed_7c.":
            pooled = F.max_pool2d(x, 3, 1, 1)
        else:
            pooled = self.avg(x)
        return torch.cat([b1, b3, bd, self.bc(p + "branch_pool", pooled)], 1)

    def block(self, name, x):
        kind = {"Mixed_5": self.block_a, "Mixed_6a": self.block_b, "Mixed_6": self.block_c, "Mixed_7a": self.block_d,
                "Mixed_7": self.block_e}
        fn = kind.get(name) or kind[name[:7]]
        return fn(name + ".", x.to(self.dtype))

    def __call__(self, x):
        """torchvision: logits (B, 1000).  fid: {dims: (B, dims)} for every dims the input is large enough for."""
        x = x.to(self.dtype)
        out = {}
        x = self.bc("Conv2d_1a_3x3", x, stride=2)
        x = self.bc("Conv2d_2a_3x3", x)
        x = self.bc("Conv2d_2b_3x3", x, padding=1)
        x = F.max_pool2d(x, 3, 2)
        out[64] = x.mean((2, 3))
        x = self.bc("Conv2d_3b_1x1", x)
        x = self.bc("Conv2d_4a_3x3", x)
        x = F.max_pool2d(x, 3, 2)
        out[192] = x.mean((2, 3))
        for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.block(name, x)
        out[768] = x.mean((2, 3))
        for name in ("Mixed_7a", "Mixed_7b", "Mixed_7c"):
            x = self.block(name, x)
        out[2048] = x.mean((2, 3))
        if self.variant == "torchvision":
            return F.linear(out[2048], self.sd["fc.weight"], self.sd["fc.bias"])
        return out


BLOCK_CASES = (("Mixed_5b", 192), ("Mixed_6a", 288), ("Mixed_6b", 768), ("Mixed_7a", 768), ("Mixed_7b", 1280),
               ("Mixed_7c", 2048))          # each block type once (E twice: the fid variant's two E blocks differ)


def prepare(images, variant, size=(299, 299), channel_order="rgb", dtype=torch.float64):
    """The input stage restated: uint8 (B,H,W,3) -> /255, or float (B,3,H,W); bilinear resize (align_corners=False), then
    2x - 1 for fid.  CPU, `dtype`."""
    if images.dtype == torch.uint8:
        x = (images.cpu().to(torch.float32) / 255).to(dtype).permute(0, 3, 1, 2)
    else:
        x = images.cpu().to(dtype)
    if channel_order == "bgr":
        x = x.flip(1)
    if size is not None:
        x = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    return 2 * x - 1 if variant == "fid" else x


# ---------------------------------------------------------------------------------------------- quality: formulas and cases
FRECHET_FULL = ((64, 200), (64, 65), (192, 400))
FRECHET_DEFICIENT = ((64, 40), (192, 100))
FRECHET_CASES = FRECHET_FULL + FRECHET_DEFICIENT
SCORE_CASES = ((20, 1), (20, 5), (23, 5), (23, 1))        # 23: not divisible by 5


def frechet_inputs(D, N, seed):
    """(mu1, sigma1, mu2, sigma2) of two seeded sets of N correlated D-wide feature rows (N <= D: rank-deficient)."""
    rng = np.random.default_rng(1234 + seed)
    out = []
    for k in range(2):
        mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D) * 0.5
        act = np.abs(rng.standard_normal((N, D)).dot(mix)) * (0.3 + 0.1 * k) + 0.05 * k
        out += [np.mean(act, axis=0), np.cov(act, rowvar=False)]
    return tuple(out)


def score_probabilities(N, K=1000, seed=0):
    """(N, K) float64 rows that are fp32 softmax outputs (as the reference stores them), peaked on different classes."""
    g = torch.Generator().manual_seed(4321 + seed + N)
    logits = torch.randn(N, K, generator=g) * 2.0
    logits[torch.arange(N), torch.randint(0, K, (N,), generator=g)] += 6.0
    return F.softmax(logits, dim=1).numpy().astype(np.float64)


def score_formula(probs, splits):
    """compute_score restated in numpy fp64 as the device computes it: per split exp(mean_i sum_j pk log(pk / qk)) with
    pk = p_i / sum(p_i), qk = py / sum(py), py = mean_i p_i; then mean and population std over the splits."""
    probs = np.asarray(probs, np.float64)
    N = probs.shape[0]
    per = N // splits
    scores = []
    for k in range(splits):
        part = probs[k * per:(k + 1) * per]
        py = part.mean(axis=0)
        qk = py / py.sum()
        kls = []
        for row in part:
            pk = row / row.sum()
            nz = pk > 0
            kls.append(np.sum(pk[nz] * np.log(pk[nz] / qk[nz])))
        scores.append(np.exp(np.mean(kls)))
    return float(np.mean(scores)), float(np.std(scores))


def pictures(n, side=64, seed=0):
    """n seeded uint8 (side, side, 3) pictures with some structure (smooth blobs + noise), as one (n, side, side, 3) tensor."""
    g = torch.Generator().manual_seed(99 + seed)
    low = torch.rand(n, 3, 8, 8, generator=g)
    img = F.interpolate(low, size=(side, side), mode="bilinear", align_corners=False) + 0.15 * torch.rand(n, 3, side, side, generator=g)
    return (img.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
