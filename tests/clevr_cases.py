"""The CLEVR input stage's cases and host restatements (tests/test_clevr_cases.py pins them on the CPU,
tests/test_gpu_clevr.py holds csrc/clevr.hip and the 4-byte pixels of csrc/preprocess.hip to them bit for bit).

`boxes_fp64` restates the reference's extract_bounding_boxes (sg2im/data/packed_clevr_dialog.py:21-77) in numpy fp64, in
its operation order; `rgb_of` is what Pillow's RGBA -> RGB conversion does (it drops the alpha byte); the resize and the
float stage are those of tests/preprocess_cases.py with CLEVR's Normalize(0.5, 0.5) (sg2im/data/utils.py:13-14)."""
import json
import os

import numpy as np

import preprocess_cases as pc

MEAN = STD = (0.5, 0.5, 0.5)
CUBE, SPHERE, CYLINDER = 1, 2, 3

OUTPUTS = [(64, 64), (30, 30)]                            # W % 4 == 0: dword / float4 stores; W % 4 != 0: the narrow ones

# name -> [(h, w, bytes per pixel)]: the pictures of one call, in order
BATCHES = {
    "mixed": [(32, 48, 4), (37, 53, 3), (64, 64, 4)],      # RGBA resized, RGB upscaled, RGBA passed through at 64 x 64
    "odd_offset": [(5, 7, 3), (32, 48, 4)],                # 105 bytes in front: the 4-byte picture starts at an odd byte
    "clevr_frame": [(320, 480, 4)],                        # CLEVR's own render size
}


def batch_id(case):
    return "%s_to_%dx%d" % (case[0], case[1][0], case[1][1])


CASES = [(name, hw) for name in BATCHES for hw in OUTPUTS]


def batch_images(name, seed=0):
    """The seeded pictures of a batch: uint8 (h, w, bytes per pixel), uniform bytes, the alpha byte included."""
    return [np.random.default_rng(1000 * seed + 100 * i + 7 * h + w + bpp).integers(0, 256, size=(h, w, bpp), dtype=np.uint8)
            for i, (h, w, bpp) in enumerate(BATCHES[name])]


def rgb_of(img):
    """The first three bytes of every pixel: Pillow's convert('RGB') of an RGBA picture; an RGB picture as it is."""
    return np.ascontiguousarray(img[..., :3])


def pack_px(images):
    """A list of (h, w, 3 | 4) uint8 arrays -> (packed bytes uint8 (N,), descriptor int64 (B, 4) = byte offset, h, w, bytes
    per pixel), back to back with no padding."""
    desc = np.zeros((len(images), 4), np.int64)
    off = 0
    for i, im in enumerate(images):
        desc[i] = (off, im.shape[0], im.shape[1], im.shape[2])
        off += im.size
    return np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images]), desc


def to_float(u8, normalize=True):
    return pc.to_float(u8, mean=MEAN if normalize else None, std=STD)


def boxes_fp64(geom, shape, rot, counts):
    """geom (B,O,5) fp64 = pixel x, pixel y, 3d x, y, z; shape (B,O) ids; rot (B,2) = (cos, sin); counts (B,) ->
    fp32 (B,O,4) = (x_min, y_min, x_max - x_min, y_max - y_min), -1 in padding rows.  Every line is one line of the
    reference, elementwise in fp64; the one rounding to fp32 is the last statement."""
    geom = np.asarray(geom, np.float64)
    shape = np.asarray(shape)
    x, y, x1, y1, z1 = (geom[..., i] for i in range(5))
    cos_theta, sin_theta = np.asarray(rot, np.float64)[:, None, 0], np.asarray(rot, np.float64)[:, None, 1]
    with np.errstate(all="ignore"):                       # padding rows are all zeros: finite, and overwritten below
        x1 = x1 * cos_theta + y1 * sin_theta
        y1 = x1 * -sin_theta + y1 * cos_theta
        height_d = 6.9 * z1 * (15 - y1) / 2.0
        height_u, width_l, width_r = height_d, height_d, height_d
        d = 9.4 + y1
        h = 6.4
        s = z1
        cyl_u = height_u * ((s * (h / d + 1)) / ((s * (h / d + 1)) - (s * (h - s) / d)))
        cyl_d = cyl_u * (h - s + d) / (h + s + d)
        cyl_l = width_l * (11 / (10 + y1))
        cube_u = height_u * (1.3 * 10 / (10 + y1))
        cyl, cube = shape == CYLINDER, shape == CUBE
        height_u = np.where(cyl, cyl_u, np.where(cube, cube_u, height_u))
        height_d = np.where(cyl, cyl_d, np.where(cube, cube_u, height_d))
        width_l = np.where(cyl, cyl_l, np.where(cube, cube_u, width_l))
        width_r = width_l
        y_min = (y - height_d) / 320.
        y_max = (y + height_u) / 320.
        x_max = (x + width_r) / 480.
        x_min = (x - width_l) / 480.
        out = np.stack([x_min, y_min, x_max - x_min, y_max - y_min], -1)
    real = np.arange(geom.shape[1])[None] < np.asarray(counts)[:, None]
    return np.where(real[..., None], out, -1.0).astype(np.float32)


# ------------------------------------------------------------------------------- a tiny folder in the reference's layout
COLORS = ["gray", "red", "blue", "green", "brown", "purple", "cyan", "yellow"]
FOLDER_MODES = ["RGBA", "RGB", "RGBA", "RGBA", "RGB"]
FOLDER_SIZES = [(32, 48), (37, 53), (64, 64), (40, 60), (64, 30)]          # (h, w)
FOLDER_COUNTS = [3, 4, 5, 6, 3]


def folder_scene(i, split="train"):
    rng = np.random.default_rng(300 + i)
    theta = float(rng.uniform(-0.6, 0.6))
    objects = []
    for o in range(FOLDER_COUNTS[i]):
        objects.append({
            "shape": ["cube", "sphere", "cylinder"][(i + o) % 3], "color": COLORS[(3 * i + o) % 8],
            "material": ["rubber", "metal"][(i + o) % 2], "size": ["small", "large"][o % 2],
            "3d_coords": [float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), [0.35, 0.7][o % 2]],
            "pixel_coords": [int(rng.integers(20, 460)), int(rng.integers(20, 300)), float(rng.uniform(7, 14))],
            "rotation": float(rng.uniform(0, 360)),
        })
    return {"image_index": 10 + i, "image_filename": "CLEVR_%s_%06d.png" % (split, i), "split": split, "objects": objects,
            "directions": {"right": [float(np.cos(theta)), float(np.sin(theta)), 0.0], "above": [0.0, 0.0, 1.0]}}


def write_folder(root, split="train", dialog=False):
    """<root>/CLEVR/CLEVR_Dialog in the reference's layout: scenes/CLEVR_<split>_scenes.json and five seeded PNGs under
    images/<split>/, RGBA and RGB mixed, scenes of 3 .. 6 objects.  dialog=True also writes clevr_dialog_<split>_raw.json
    whose entry i names the picture of scene 4 - i (under images/<split>/ too): the dialog file decides, when it exists.
    Returns (base, scenes, {file name: the decoded pixels})."""
    from PIL import Image
    base = os.path.join(root, "CLEVR", "CLEVR_Dialog")
    os.makedirs(os.path.join(base, "scenes"), exist_ok=True)
    os.makedirs(os.path.join(base, "images", split), exist_ok=True)
    scenes = [folder_scene(i, split) for i in range(5)]
    pixels = {}
    for i, (s, mode, (h, w)) in enumerate(zip(scenes, FOLDER_MODES, FOLDER_SIZES)):
        px = np.random.default_rng(70 + i).integers(0, 256, size=(h, w, len(mode)), dtype=np.uint8)
        Image.fromarray(px, mode).save(os.path.join(base, "images", split, s["image_filename"]))
        pixels[s["image_filename"]] = px
    with open(os.path.join(base, "scenes", "CLEVR_%s_scenes.json" % split), "w") as f:
        json.dump({"info": {"split": split}, "scenes": scenes}, f)
    if dialog:
        with open(os.path.join(base, "clevr_dialog_%s_raw.json" % split), "w") as f:
            json.dump([{"split": split, "image_filename": scenes[4 - i]["image_filename"], "dialogs": []} for i in range(5)], f)
    return base, scenes, pixels
