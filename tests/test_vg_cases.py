"""The Visual Genome input stage's host restatement against the reference's recorded samples (CPU; tests/vg_cases.py,
tests/golden/vg_samples.npz), and the folder dataset's host half.  No tolerance anywhere: the boxes are four fp64 divisions
rounded once to fp32, the rest is integers."""
import importlib.util
import json
import os
import platform
import random
import sys

import numpy as np
import pytest

import vg_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = list(range(6))


def _dataset(base, si=None, split="train", **kw):
    from canonicalsg2im_amd.sg2im.data.packed_vg import PackedVGDataset
    if si is not None:
        s = vc.golden()[0]["settings"][si]
        kw.update(max_objects=s["max_objects"], use_orphaned_objects=bool(s["use_orphaned_objects"]),
                  include_relationships=bool(s["include_relationships"]))
    return PackedVGDataset(os.path.join(base, split + ".npz"), os.path.join(base, "images"), os.path.join(base, "vocab.json"),
                           **kw)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return vc.write_folder(str(tmp_path_factory.mktemp("vg")))


def test_the_golden_has_the_cases_it_is_meant_to_have():
    meta, g = vc.golden()
    assert len(meta["settings"]) == len(SETTINGS) and g["object_names"].shape == (4, 24) and g["relationship_subjects"].shape == (4, 16)
    assert g["objects_per_image"].tolist() == [5, 12, 24, 9] and g["relationships_per_image"].tolist() == [3, 16, 7, 0]
    assert g["sizes"].tolist() == [[333, 500], [481, 640], [200, 201], [1024, 683]]
    want = {(100, 1, 1, 0), (10, 1, 1, 0), (100, 0, 1, 0), (100, 1, 0, 0), (100, 1, 1, 1), (10, 1, 1, 1)}
    assert {(s["max_objects"], s["use_orphaned_objects"], s["include_relationships"], s["learned_transitivity"])
            for s in meta["settings"]} == want
    assert g["s0_n"].tolist() == [6, 13, 25, 10]                         # every object and __image__
    assert g["s1_n"].tolist() == [6, 11, 11, 10]                         # max_objects = 10: 11 rows, the reference's off-by-one
    assert meta["settings"][2]["samples"] == [0, 1, 2]                   # the reference cannot run sample 3 without orphans
    boxes, sizes = g["object_boxes"], g["sizes"]
    for i in range(4):
        assert boxes[i, 0, 0] == 0 and boxes[i, 1, 2] == sizes[i, 1]
        assert boxes[i, 2, 0] + boxes[i, 2, 2] > sizes[i, 1] and boxes[i, 2, 1] + boxes[i, 2, 3] > sizes[i, 0]
    real = g["s0_boxes"][..., 0] >= 0
    assert float((g["s0_boxes"][..., 0] + g["s0_boxes"][..., 2])[real].max()) > 1.0      # nothing clips a box to the picture


@pytest.mark.parametrize("si", SETTINGS, ids=vc.setting_id)
def test_select_and_restatement_equal_the_reference(folder, si):
    """`select` under the golden's seed picks the reference's objects in the reference's order and keeps its annotated rows;
    the numpy restatement of csg_vg_rows over them equals the collate's objects and boxes bit for bit."""
    meta, g = vc.golden()
    s = meta["settings"][si]
    ds = _dataset(folder[0], si)
    why = "the golden was made with Python %s, this is %s: set order and random.sample are pinned per interpreter version" % (
        meta["python"], platform.python_version())
    picks = vc.select_all(ds, si)
    n = g["s%d_n" % si]
    assert [len(chosen) + 1 for chosen, _ in picks] == n.tolist(), why
    for b, (i, (chosen, rows)) in enumerate(zip(s["samples"], picks)):
        assert len(set(chosen)) == len(chosen) and all(0 <= c < g["objects_per_image"][i] for c in chosen)
        assert g["object_names"][i, chosen].tolist() == g["s%d_objs" % si][b, :n[b] - 1].tolist(), why
        assert {tuple(r) for r in rows} == vc.golden_annotated(g, si, b, ds.vocab), why
        r = int(g["relationships_per_image"][i])                           # in file order, duplicates kept, remapped to positions
        in_file = zip(g["relationship_subjects"][i, :r], g["relationship_predicates"][i, :r], g["relationship_objects"][i, :r])
        want = [[chosen.index(a), int(p), chosen.index(c)] for a, p, c in in_file if a in chosen and c in chosen]
        assert rows == (want if s["include_relationships"] else [])
    rows, counts = vc.padded_rows(g, s["samples"], [chosen for chosen, _ in picks])
    sizes = g["sizes"][s["samples"]]
    objs, boxes = vc.with_image_row(*vc.rows_fp64(rows, sizes, counts, ds.num_objects))
    want_objs, want_boxes = g["s%d_objs" % si].astype(np.int64), g["s%d_boxes" % si]
    assert objs.shape == want_objs.shape and np.array_equal(objs, want_objs)
    differing = int((boxes.view(np.uint32) != want_boxes.view(np.uint32)).any(-1).sum())
    print("%s: %d of %d box rows differ from the reference's bits" % (vc.setting_id(si), differing, boxes.shape[0] * boxes.shape[1]))
    assert boxes.dtype == np.float32 and differing == 0
    # a plain fp32 division gives the same bits here (values below 2^24), as csrc/vg.hip's comment says
    real = np.arange(rows.shape[1])[None] < counts[:, None]
    f32 = rows[..., 1].astype(np.float32) / sizes[:, None, 1].astype(np.float32)
    assert np.array_equal(f32[real], boxes[:, :-1, 0][real])


def test_select_without_orphans_on_a_sample_without_relationships(folder):
    ds = _dataset(folder[0], 2)
    assert ds.select(3, random.Random(0)) == ([], [])
    assert _dataset(folder[0], 0).select(3, random.Random(0))[1] == []


def test_dataset_on_a_tiny_folder(folder, tmp_path):
    from canonicalsg2im_amd.sg2im.data.packed_vg import PackedVGDataset, load_split, split_file
    base, decoded = folder
    ds = _dataset(base)
    v = ds.vocab
    # ---- vocabulary: vocab.json plus what the reference's constructor adds (:60-65)
    assert v["attributes"] == {"objects": v["object_name_to_idx"]} and list(v["attributes"]) == ["objects"]
    assert v["reverse_attributes"]["objects"][0] == "__image__" and len(v["reverse_attributes"]["objects"]) == 179
    assert len(v["pred_idx_to_name"]) == 46 and v["pred_name_to_idx"]["__surrounding__"] == 7 and ds.num_objects == 179
    assert {"object_name_to_idx", "object_idx_to_name", "pred_name_to_idx", "pred_idx_to_name"} <= set(v)
    # ---- samples
    assert len(ds) == 4 and ds.image_ids == [100, 101, 2317, 7] and ds.image_paths == vc.FOLDER_FILES
    assert all(ds.data[k].dtype == np.int32 for k in vc.TABLES) and set(ds.data) == set(vc.TABLES)     # image_ids ignored
    with ds.open(3) as im:
        assert im.size == (683, 1024) and im.mode == "RGB"
    px, rows, rel, image_id = ds.load(1, random.Random(3))
    assert np.array_equal(px, decoded[1]) and px.shape == (481, 640, 3) and image_id == 101           # the L picture, as RGB
    assert rows.shape == (12, 5) and rows.dtype == np.int32 and rel.shape[1] == 3 and rel.dtype == np.int64
    # ---- filters
    assert _dataset(base, min_objects=9).image_ids == [101, 2317, 7]
    kept = _dataset(base, min_objects=10)
    assert kept.image_ids == [101, 2317] and kept.data["relationships_per_image"].tolist() == [16, 7]
    assert kept.data["object_boxes"].shape == (2, 24, 4) and _dataset(base, min_objects=25).image_ids == []
    assert len(_dataset(base, max_samples=3)) == 3 and len(_dataset(base, max_samples=9)) == 4
    # ---- image_paths as bytes; the other extension; a missing key
    other = vc.write_folder(str(tmp_path), split="val", paths_as_bytes=True)[0]
    assert _dataset(other, split="val").image_paths == vc.FOLDER_FILES
    assert split_file(os.path.join(other, "val.h5")) == os.path.join(other, "val.npz")
    assert split_file(os.path.join(other, "train.h5")) is None and split_file(os.path.join(other, "val.txt")) is None
    assert load_split(os.path.join(other, "val.h5"))[1] == vc.FOLDER_FILES
    np.savez(os.path.join(other, "short.npz"), object_names=np.zeros((1, 2)))
    with pytest.raises(KeyError, match="short.npz lacks object_boxes"):
        load_split(os.path.join(other, "short.npz"))
    # ---- refusals
    with pytest.raises(NotImplementedError, match="mask_size must be 0.*masks = None"):
        _dataset(base, mask_size=16)
    for kw in ({"use_transitivity": True}, {"use_converse": True}):
        with pytest.raises(NotImplementedError, match="as in the reference"):
            _dataset(base, **kw)
    moved = dict(vc.vocab())
    moved["object_name_to_idx"] = dict(moved["object_name_to_idx"], __image__=5)
    with open(os.path.join(other, "moved.json"), "w") as f:
        json.dump(moved, f)
    with pytest.raises(ValueError, match="__image__ must be object 0"):
        PackedVGDataset(os.path.join(other, "val.npz"), os.path.join(other, "images"), os.path.join(other, "moved.json"))


def test_an_h5_split_without_h5py_names_the_converter(tmp_path, monkeypatch):
    from canonicalsg2im_amd.sg2im.data.packed_vg import load_split
    path = tmp_path / "train.h5"
    path.write_bytes(b"\x89HDF\r\n\x1a\n")
    monkeypatch.setitem(sys.modules, "h5py", None)                       # `import h5py` raises ImportError, wherever this runs
    with pytest.raises(ImportError, match=r"train\.h5 is an HDF5 file.*tools/vg_h5_to_npz\.py"):
        load_split(str(path))


def test_converter_handles_its_arguments_without_h5py(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("vg_h5_to_npz", os.path.join(ROOT, "tools", "vg_h5_to_npz.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit) as e:
        tool.main(["--help"])
    assert e.value.code == 0 and "split file" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        tool.main([str(tmp_path / "nowhere.h5")])
    assert e.value.code == 2 and "no such file" in capsys.readouterr().err


def test_command_line_finds_the_folder_or_falls_back(folder, tmp_path):
    from canonicalsg2im_amd.scripts.train import build_parser, folder_dataset
    base = folder[0]
    root = os.path.dirname(base)
    parse = build_parser().parse_args
    ds = folder_dataset(parse(["--dataset", "packed_vg", "--dataroot", root, "--image_size", "64,64"]), "train")
    assert ds.image_ids == [2317] and ds.max_objects == 100 and ds.image_size == (64, 64)      # min_objects = 16, as the reference
    assert ds.image_dir == os.path.join(base, "images")
    args = parse(["--dataset", "packed_vg", "--dataroot", root, "--min_objects", "0", "--max_objects", "10",
                  "--num_train_samples", "3", "--vg_use_orphaned_objects", "0", "--include_relationships", "0"])
    ds = folder_dataset(args, "train")
    assert len(ds) == 3 and ds.max_objects == 10 and not ds.use_orphaned_objects and not ds.include_relationships
    assert folder_dataset(args, "val") is None                                     # no val split file: synthetic validation
    assert folder_dataset(parse(["--dataset", "packed_vg", "--dataroot", str(tmp_path / "nowhere")]), "train") is None
    # the flags win where their paths exist
    split = str(tmp_path / "two.npz")
    _, g = vc.golden()
    np.savez(split, image_paths=np.asarray(vc.FOLDER_FILES[:2]), **{k: g[k][:2] for k in vc.TABLES})
    args = parse(["--dataset", "packed_vg", "--dataroot", str(tmp_path / "nowhere"), "--min_objects", "1", "--train_h5", split,
                  "--vg_image_dir", os.path.join(base, "images"), "--vocab_json", os.path.join(base, "vocab.json")])
    assert folder_dataset(args, "train").image_ids == [100, 101]
    with pytest.raises(NotImplementedError, match="mask_size must be 0"):
        folder_dataset(parse(["--dataset", "packed_vg", "--dataroot", root, "--mask_size", "16"]), "train")
    with pytest.raises(NotImplementedError, match="as in the reference"):
        folder_dataset(parse(["--dataset", "packed_vg", "--dataroot", root, "--use_transitivity", "1"]), "train")
