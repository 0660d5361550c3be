"""The input stage's cases and its host restatements (tests/test_preprocess_cases.py pins them on the CPU,
tests/test_gpu_preprocess.py holds csrc/preprocess.hip to them bit for bit).

`pil_resize_u8` restates Pillow's 8-bit `Image.resize((W, H), BILINEAR)` — what torchvision's `T.Resize` is on a PIL
image (sg2im/data/packed_coco.py:269) — in numpy; `to_float` is `T.ToTensor()` followed by `T.Normalize(mean, std)`
(:269-272) as the three fp32 operations torch does on the host."""
import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)                 # sg2im/data/utils.py:6-7
IMAGENET_STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22                                   # 32 - 8 - 2: Pillow's fixed-point coefficients
MAX_FILTERSCALE = 64                                  # the device's supported shrink per axis (include/csg_hip.h)

# (source h, source w, H, W, what it exercises)
CASES = [
    (480, 640, 256, 256, "the workload's ordinary downscale"),
    (427, 640, 64, 64, "10x shrink, 21 taps"),
    (37, 53, 64, 64, "upscale (fs = 1, 2-3 taps); 159-byte rows"),
    (500, 333, 256, 256, "portrait; different factors per axis"),
    (64, 64, 64, 64, "both passes skipped"),
    (300, 64, 64, 64, "horizontal pass skipped"),
    (17, 1000, 8, 8, "125x shrink, 251 taps: beyond the device's range, refused there"),
    (640, 480, 128, 128, "landscape stored tall; 128 x 128"),
]

# rows beyond the table, at the edge of the device's range: the full tap-major coefficient table of the horizontal pass
LIMIT_CASES = [
    (512, 512, 8, 8, "64x shrink on both axes: fs = 64 exactly: 128 taps, the most the range can produce"),
    (500, 500, 8, 8, "62.5x shrink: a fractional scale next to the limit, 125 taps"),
]


def supported(h, w, H, W):
    """Inside the device's stated range: sides 1 .. 8192 and a shrink of at most MAX_FILTERSCALE per axis."""
    return all(1 <= s <= 8192 for s in (h, w, H, W)) and h <= MAX_FILTERSCALE * H and w <= MAX_FILTERSCALE * W


def case_id(case):
    return "%dx%d_to_%dx%d" % case[:4]


def case_image(case, seed=0):
    """uint8 (h, w, 3), seeded uniform bytes: random pixels are the worst case for rounding."""
    h, w = case[:2]
    return np.random.default_rng(1000 * seed + 7 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def axis_coefficients(in_size, out_size):
    """Per output index: (first tap, int32 coefficients) of Pillow's bilinear filter, in its fp64 operation order."""
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = fs                                      # the bilinear filter's support is 1.0
    ss = 1.0 / fs
    out = []
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), in_size)
        ws = []
        ww = 0.0
        for x in range(xmax - xmin):
            a = abs((x + xmin - c + 0.5) * ss)
            w = 1.0 - a if a < 1.0 else 0.0
            ws.append(w)
            ww += w
        k = []
        for w in ws:
            if ww != 0.0:
                w = w / ww
            k.append(int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)))
        out.append((xmin, np.asarray(k, np.int64)))
    return out


def _resample(img, out_size, axis):
    """One pass along `axis` of a (h, w, 3) uint8 image -> uint8."""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for xx, (xmin, k) in enumerate(axis_coefficients(img.shape[0], out_size)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, img[xmin:xmin + k.shape[0]], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize_u8(img, H, W):
    """Pillow's `Image.fromarray(img).resize((W, H), Image.BILINEAR)` for an 8-bit RGB image (h, w, 3) -> (H, W, 3):
    the horizontal pass first, into a uint8 intermediate, then the vertical pass; a pass that keeps its size is skipped."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.shape[1] != W:
        img = _resample(img, W, 1)
    if img.shape[0] != H:
        img = _resample(img, H, 0)
    return np.ascontiguousarray(img)


def to_float(u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 (..., H, W, 3) -> fp32 (..., 3, H, W): ToTensor's `.float().div(255)`, then Normalize's `.sub(mean).div(std)`
    with mean and std as fp32 tensors, on the CPU.  mean = None: ToTensor alone (normalize_images=False)."""
    t = torch.as_tensor(np.ascontiguousarray(u8))
    t = t.movedim(-1, -3).contiguous().float().div(255)
    if mean is None:
        return t
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1, 1)
    return t.sub(m).div(s)


def pack_images(images):
    """A list of (h, w, 3) uint8 arrays -> (packed bytes uint8 (N,), descriptor int64 (B, 3) = byte offset, h, w)."""
    desc = np.zeros((len(images), 3), np.int64)
    off = 0
    for i, im in enumerate(images):
        desc[i] = (off, im.shape[0], im.shape[1])
        off += im.size
    return np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images]), desc
