#!/usr/bin/env python
"""Generate tests/golden/clevr_boxes.npz by running the REAL reference's extract_bounding_boxes
(sg2im/data/packed_clevr_dialog.py:21-77) on seeded CLEVR-like scenes.

Needs a checkout of the reference, named on the command line.  The module's imports need cv2 and matplotlib, so the ONE function
is taken from the module's source by its AST and executed on its own: it uses no name but builtins.  Nothing of the
reference travels: the output is the scenes' raw numbers and the fp32 boxes the reference makes of them
(`torch.FloatTensor(list(zip(x, y, w, h)))`, :188-189,203) + JSON metadata.

    python tests/golden/make_golden_clevr.py REFERENCE_CHECKOUT
"""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join("sg2im", "data", "packed_clevr_dialog.py")       # under the reference checkout
SHAPES = ["cube", "sphere", "cylinder"]                 # ids 1, 2, 3 (:121)
COUNTS = [1, 10, 3, 4, 5, 6, 7, 8, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10]      # 183 objects, 22 scenes


def reference_function(checkout):
    tree = ast.parse(open(os.path.join(checkout, SOURCE)).read(), SOURCE)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "extract_bounding_boxes"]
    assert len(fn) == 1
    scope = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), SOURCE, "exec"), scope)
    return scope["extract_bounding_boxes"]


def make_scenes(seed=20):
    """CLEVR's ranges: 3d x, y in [-3, 3] (y on both sides of 0), z = the size (0.35 small, 0.7 large), integer pixel
    coordinates inside the 480 x 320 frame, a camera rotated by a seeded angle (CLEVR jitters it per scene); scene 2 is
    CLEVR's unjittered identity-like direction with y1 exactly 0 once."""
    rng = np.random.default_rng(seed)
    scenes = []
    for s, n in enumerate(COUNTS):
        theta = 0.0 if s == 2 else float(rng.uniform(-np.pi, np.pi))
        right = [float(np.cos(theta)), float(np.sin(theta)), 0.0]
        objects = []
        for o in range(n):
            shape = SHAPES[(s + o) % 3] if s else "cylinder"
            z = [0.35, 0.7][int(rng.integers(0, 2))]
            xyz = [float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), z]
            if s == 2 and o == 0:
                xyz[1] = 0.0
            pixel = [int(rng.integers(20, 460)), int(rng.integers(20, 300)), float(rng.uniform(7, 14))]
            objects.append({"shape": shape, "pixel_coords": pixel, "3d_coords": xyz})
        scenes.append({"objects": objects, "directions": {"right": right}})
    return scenes


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    extract = reference_function(sys.argv[1])
    scenes = make_scenes()
    O = max(COUNTS)
    B = len(scenes)
    geom = np.zeros((B, O, 5), np.float64)
    shape = np.zeros((B, O), np.int64)
    rot = np.zeros((B, 2), np.float64)
    counts = np.asarray(COUNTS, np.int64)
    boxes = np.full((B, O, 4), -1.0, np.float32)
    for b, scene in enumerate(scenes):
        x, y, w, h = extract(scene)
        boxes[b, :counts[b]] = torch.FloatTensor(list(zip(x, y, w, h))).numpy()
        rot[b] = scene["directions"]["right"][:2]
        for o, obj in enumerate(scene["objects"]):
            geom[b, o] = obj["pixel_coords"][:2] + obj["3d_coords"]
            shape[b, o] = 1 + SHAPES.index(obj["shape"])
    x1 = geom[..., 2] * rot[:, None, 0] + geom[..., 3] * rot[:, None, 1]
    y1 = x1 * -rot[:, None, 1] + geom[..., 3] * rot[:, None, 0]                   # the rotated y1: both signs must occur
    real = np.arange(O)[None] < counts[:, None]
    meta = {"source": "sg2im/data/packed_clevr_dialog.py:21-77 extract_bounding_boxes, run by make_golden_clevr.py",
            "objects": int(counts.sum()), "scenes": B, "shape_ids": {"cube": 1, "sphere": 2, "cylinder": 3},
            "geom": "pixel x, pixel y, 3d x, 3d y, 3d z", "rot": "directions['right'][:2]",
            "y1_negative": int((y1[real] < 0).sum()), "y1_positive": int((y1[real] > 0).sum())}
    assert meta["y1_negative"] > 20 and meta["y1_positive"] > 20 and set(shape[real]) == {1, 2, 3}
    out = os.path.join(HERE, "clevr_boxes.npz")
    np.savez_compressed(out, geom=geom, shape=shape, rot=rot, counts=counts, boxes=boxes,
                        __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    print(out, os.path.getsize(out), "bytes", meta, file=sys.stderr)


if __name__ == "__main__":
    main()
