"""The CLEVR input stage's host restatements against what they restate (CPU; tests/clevr_cases.py), and the folder dataset's
host half."""
import json
import os

import numpy as np
import pytest
import torch

import clevr_cases as cc
import preprocess_cases as pc
from conftest import load_golden


def test_box_restatement_equals_the_reference_bit_for_bit():
    """tests/golden/clevr_boxes.npz holds what the reference's extract_bounding_boxes made of 183 seeded objects in 22 scenes.
    Only + - * / in fp64 and one rounding to fp32 occur on either side: equality, no tolerance."""
    meta, g = load_golden("clevr_boxes")
    counts = g["counts"].numpy()
    real = np.arange(g["shape"].shape[1])[None] < counts[:, None]
    shape = g["shape"].numpy()
    assert meta["objects"] == int(counts.sum()) == 183 and len(counts) == 22
    assert set(shape[real]) == {cc.CUBE, cc.SPHERE, cc.CYLINDER}
    assert meta["y1_negative"] > 20 and meta["y1_positive"] > 20
    assert 1 in counts and counts.max() == 10
    assert set(g["geom"].numpy()[real][:, 4]) == {0.35, 0.7}
    assert not np.allclose(g["rot"].numpy()[:, 0], 1.0)
    got = cc.boxes_fp64(g["geom"].numpy(), shape, g["rot"].numpy(), counts)
    want = g["boxes"].numpy()
    differing = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(-1))
    print("box restatement: %d of %d rows differ from the reference's bits" % (len(differing), got.shape[0] * got.shape[1]))
    assert got.dtype == np.float32 and len(differing) == 0, differing[:5]
    assert (want[~real] == -1).all() and (want[real][:, 2:] > 0).all()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.batch_id)
def test_resize_of_the_first_three_bytes_is_pillows_convert_then_resize(case):
    """Pillow's RGBA -> RGB conversion drops the alpha byte and does nothing else: pil_resize_u8 on img[..., :3] equals
    `convert('RGB').resize(...)` of the installed Pillow, 0 differing bytes on every picture of every case."""
    Image = pytest.importorskip("PIL.Image")
    name, (H, W) = case
    for img in cc.batch_images(name):
        pil = Image.fromarray(img, "RGBA" if img.shape[2] == 4 else "RGB")
        assert np.array_equal(np.asarray(pil.convert("RGB")), cc.rgb_of(img))
        want = np.asarray(pil.convert("RGB").resize((W, H), Image.BILINEAR))
        got = pc.pil_resize_u8(cc.rgb_of(img), H, W)
        differing = int((want != got).sum())
        print("%s %s: %d differing bytes of %d" % (cc.batch_id(case), img.shape, differing, want.size))
        assert differing == 0


def test_the_table_has_the_cases_it_is_meant_to_have():
    packed, desc = cc.pack_px(cc.batch_images("odd_offset"))
    assert desc[1, 0] % 2 == 1 and desc[1, 3] == 4 and packed.shape[0] == 105 + 4 * 32 * 48
    assert [b[2] for b in cc.BATCHES["mixed"]] == [4, 3, 4] and cc.BATCHES["mixed"][2][:2] == (64, 64)
    assert cc.BATCHES["clevr_frame"] == [(320, 480, 4)]
    assert {W % 4 for _, (H, W) in cc.CASES} == {0, 2}
    for (off, h, w, bpp), im in zip(desc, cc.batch_images("odd_offset")):
        assert np.array_equal(packed[off:off + bpp * h * w].reshape(h, w, bpp), im)


def test_to_float_is_torchvisions_normalize_half_half():
    """ToTensor + Normalize(0.5, 0.5) as torch computes them on the host: (byte / 255 - 0.5) / 0.5 in three fp32 operations."""
    u8 = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().float().div(255)
    assert torch.equal(cc.to_float(u8), t.sub(0.5).div(0.5))
    assert torch.equal(cc.to_float(u8, normalize=False), t)


# ------------------------------------------------------------------------------------------------ the dataset's host half
def _dataset(base, split="train", **kw):
    from canonicalsg2im_amd.sg2im.data.packed_clevr import PackedClevrDataset
    return PackedClevrDataset(os.path.join(base, "scenes", "CLEVR_%s_scenes.json" % split), os.path.join(base, "images"),
                              dialog_json=os.path.join(base, "clevr_dialog_%s_raw.json" % split), **kw)


def test_dataset_on_a_tiny_folder(tmp_path):
    pytest.importorskip("PIL")
    from canonicalsg2im_amd.sg2im.data.packed_clevr import PackedClevrDataset, clevr_vocab
    base, scenes, pixels = cc.write_folder(str(tmp_path))
    ds = _dataset(base)
    # ---- vocabulary: the reference's (packed_clevr_dialog.py:113-143)
    v = ds.vocab
    assert v["use_object_embedding"] is False
    assert list(v["attributes"]) == ["shape", "color", "material", "size"]
    assert [len(t) for t in v["attributes"].values()] == [4, 9, 3, 3]
    assert v["attributes"]["shape"] == {"__image__": 0, "cube": 1, "sphere": 2, "cylinder": 3}
    assert v["attributes"]["material"] == {"__image__": 0, "rubber": 1, "metal": 2}
    assert v["reverse_attributes"]["color"][8] == "yellow" and v["reverse_attributes"]["size"][2] == "large"
    names = v["object_name_to_idx"]
    assert list(names)[:6] == ["__image__", "cube_1", "sphere_2", "cylinder_3", "__image___4", "gray_5"]
    assert len(names) == 19 and names["large_18"] == 18 and names["__image___16"] == 16
    assert v["object_idx_to_name"] == {i: n for n, i in names.items()}
    assert v["pred_idx_to_name"] == ["__padding__", "__in_image__", "__below__", "__above__", "__left of__", "__right of__",
                                     "__inside__", "__surrounding__"]
    assert v == clevr_vocab()
    # ---- samples: column order shape, color, material, size; image_id = image_index; the scene record names the picture
    assert len(ds) == 5 and ds.image_ids == [10, 11, 12, 13, 14]
    assert ds.image_paths[1] == os.path.join("train", "CLEVR_train_000001.png")
    px, objs, geom, rot, image_id = ds.load(1)
    assert image_id == 11 and np.array_equal(px, pixels["CLEVR_train_000001.png"])             # an RGB file as it is
    assert np.array_equal(ds.load(0)[0], pixels["CLEVR_train_000000.png"][..., :3])            # an RGBA file: alpha dropped
    rows = scenes[1]["objects"]
    assert objs.dtype == torch.int64 and tuple(objs.shape) == (4, 4)
    assert objs.tolist() == [[v["attributes"][a][o[a]] for a in ("shape", "color", "material", "size")] for o in rows]
    assert geom.dtype == torch.float64 and geom.tolist() == [o["pixel_coords"][:2] + o["3d_coords"] for o in rows]
    assert rot.tolist() == scenes[1]["directions"]["right"][:2]
    # ---- filters: dense_scenes is strict on both sides, max_samples caps the length, nothing else is applied
    assert [len(s["objects"]) for s in scenes] == cc.FOLDER_COUNTS == [3, 4, 5, 6, 3]
    assert _dataset(base, dense_scenes=True, min_objects=3, max_objects=6).image_ids == [11, 12]
    assert _dataset(base, dense_scenes=True, min_objects=2, max_objects=7).image_ids == [10, 11, 12, 13, 14]
    assert _dataset(base, dense_scenes=True, min_objects=10, max_objects=10).image_ids == []
    assert len(_dataset(base, max_samples=2)) == 2 and len(_dataset(base, max_samples=9)) == 5
    # ---- the dialog file decides the picture when it exists, entry by entry, and survives the dense filter by index
    cc.write_folder(str(tmp_path), dialog=True)
    with_dialog = _dataset(base)
    assert with_dialog.image_paths == [os.path.join("train", "CLEVR_train_%06d.png" % (4 - i)) for i in range(5)]
    assert with_dialog.image_ids == [10, 11, 12, 13, 14]
    assert np.array_equal(with_dialog.load(0)[0], pixels["CLEVR_train_000004.png"])
    dense = _dataset(base, dense_scenes=True, min_objects=3, max_objects=6)
    assert dense.image_paths == [os.path.join("train", "CLEVR_train_%06d.png" % i) for i in (3, 2)]
    # ---- a directory of the pictures themselves
    flat = PackedClevrDataset(os.path.join(base, "scenes", "CLEVR_train_scenes.json"), os.path.join(base, "images", "train"),
                              split_dirs=False)
    assert flat.image_paths[2] == "CLEVR_train_000002.png" and np.array_equal(flat.load(2)[0], ds.load(2)[0])
    # ---- masks: refused, and the message says why
    with pytest.raises(NotImplementedError, match="mask_size must be 0.*masks = None"):
        _dataset(base, mask_size=16)


def test_command_line_finds_the_folder_or_falls_back(tmp_path):
    pytest.importorskip("PIL")
    from canonicalsg2im_amd.scripts.train import build_parser, folder_dataset
    base, scenes, _ = cc.write_folder(str(tmp_path))
    parse = build_parser().parse_args
    args = parse(["--dataset", "packed_clevr", "--dataroot", str(tmp_path), "--image_size", "64,64", "--num_train_samples", "4"])
    ds = folder_dataset(args, "train")
    assert len(ds) == 4 and ds.image_size == (64, 64) and ds.image_dir == os.path.join(base, "images")
    assert folder_dataset(args, "val") is None                                    # no images/val: synthetic validation
    assert folder_dataset(parse(["--dataset", "packed_clevr", "--dataroot", str(tmp_path / "nowhere")]), "train") is None
    assert folder_dataset(parse(["--dataset", "packed_vg", "--dataroot", str(tmp_path)]), "train") is None
    with pytest.raises(NotImplementedError, match="mask_size must be 0"):
        folder_dataset(parse(["--dataset", "packed_clevr", "--dataroot", str(tmp_path), "--mask_size", "16"]), "train")
    # the override flags: another scenes file, and the directory of the pictures themselves
    other = str(tmp_path / "three.json")
    with open(other, "w") as f:
        json.dump({"scenes": scenes[:3]}, f)
    args = parse(["--dataset", "packed_clevr", "--dataroot", str(tmp_path / "nowhere"), "--clevr_train_scenes_json", other,
                  "--clevr_train_image_dir", os.path.join(base, "images", "train"), "--dense_scenes", "1",
                  "--min_objects", "3", "--max_objects", "6"])
    ds = folder_dataset(args, "train")
    assert ds.image_ids == [11, 12] and ds.image_paths == ["CLEVR_train_000001.png", "CLEVR_train_000002.png"]
    with ds.open(0) as im:
        assert im.size == (53, 37)
