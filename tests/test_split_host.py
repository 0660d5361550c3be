"""The host side of the split walk (canonicalsg2im_amd/split.py) without a device: the file writer's threads, queue and
errors, the rows of layouts.json, the id <-> name tables, the host checks of generate_layouts and the command line's
refusals, all of which come before any launch."""
import json
import os
import queue
import struct
import threading

import numpy as np
import pytest
import torch


def _pictures(n, h=12, w=20, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3, h, w), dtype=np.uint8)


def _writer_threads():
    return [t for t in threading.enumerate() if t.name.startswith("csg-file-writer")]


# ------------------------------------------------------------------------------------------------- 1. the file writer
@pytest.mark.parametrize("threads", [1, 3])
def test_files_decode_to_the_submitted_arrays(tmp_path, threads):
    from PIL import Image

    from canonicalsg2im_amd.split import FileWriter
    pics = _pictures(7)
    w = FileWriter(threads, "png")
    assert w.num_threads == threads and len(_writer_threads()) == threads
    for i, p in enumerate(pics):
        w.submit(p, str(tmp_path / ("%d.png" % i)))
    w.drain()
    w.close()
    w.close()                                               # a second close is a no-op
    assert not _writer_threads()
    for i, p in enumerate(pics):
        got = np.asarray(Image.open(tmp_path / ("%d.png" % i)))
        assert got.shape == (12, 20, 3) and np.array_equal(got.transpose(2, 0, 1), p)
    with pytest.raises(RuntimeError, match="after close"):
        w.submit(pics[0], str(tmp_path / "late.png"))


def test_jpg_is_written_at_quality_95_and_other_formats_are_refused(tmp_path):
    from PIL import Image

    from canonicalsg2im_amd.split import FORMATS, FileWriter
    assert FORMATS == {"png": {}, "jpg": {"quality": 95}}
    smooth = np.broadcast_to(np.arange(0, 240, 12, dtype=np.uint8), (3, 12, 20)).copy()
    w = FileWriter(2, "jpg")
    w.submit(smooth, str(tmp_path / "5.jpg"))
    w.close()
    with Image.open(tmp_path / "5.jpg") as im:
        assert im.format == "JPEG" and im.size == (20, 12)
        assert np.abs(np.asarray(im).transpose(2, 0, 1).astype(int) - smooth).max() <= 8     # lossy, but this picture
    with pytest.raises(ValueError, match="'png' or 'jpg'.*'bmp'"):
        FileWriter(1, "bmp")
    with pytest.raises(ValueError, match="at least 1"):
        FileWriter(0, "png")
    many = FileWriter(99, "png")                            # capped, never sized from the machine
    assert many.num_threads == 16
    many.close()


def test_a_path_inside_a_regular_file_makes_close_raise_and_leaves_no_thread(tmp_path):
    from canonicalsg2im_amd.split import FileWriter
    (tmp_path / "gt").write_text("a file where a directory is expected")
    pics = _pictures(4)
    w = FileWriter(3, "png")
    w.submit(pics[0], str(tmp_path / "0.png"))
    w.submit(pics[1], str(tmp_path / "gt" / "1.png"))
    with pytest.raises((NotADirectoryError, FileNotFoundError)) as first:
        w.drain()
    with pytest.raises(type(first.value)):                  # after an error nothing more is submitted
        w.submit(pics[2], str(tmp_path / "2.png"))
    with pytest.raises(type(first.value)) as again:
        w.close()
    assert again.value is first.value and not _writer_threads()
    assert not (tmp_path / "2.png").exists()
    quiet = FileWriter(1, "png")
    quiet.submit(pics[3], str(tmp_path / "gt" / "3.png"))
    quiet.close(reraise=False)                              # for a caller that is already raising something else
    assert quiet.error is not None and not _writer_threads()


def test_a_full_queue_blocks_submit_and_does_not_grow(tmp_path):
    from canonicalsg2im_amd.split import FileWriter
    gate, started = threading.Event(), threading.Event()
    done = []

    def encode(array, path):
        started.set()
        gate.wait()
        done.append(path)

    w = FileWriter(1, "png", queue_size=2, encode=encode)
    w.submit(None, "a")
    started.wait()                                          # the one thread holds job a; the queue is empty
    w.submit(None, "b")
    w.submit(None, "c")
    assert w.jobs.full() and w.jobs.qsize() == 2
    with pytest.raises(queue.Full):                         # a blocking submit would wait here: there is no room
        w.submit(None, "d", block=False)
    assert w.jobs.qsize() == 2
    gate.set()
    w.submit(None, "d")                                     # room again: goes through
    w.close()
    assert done == ["a", "b", "c", "d"] and not _writer_threads()


# ------------------------------------------------------------------------------------------------- 2. rows and names
def _bits(x):
    return struct.pack("<f", x)


def test_layout_rows_round_trip_fp32_bit_patterns(tmp_path):
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 2 ** 32, size=4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    vals = np.concatenate([raw[np.isfinite(raw)], np.float32([0.0, -0.0, 1e-45, -1.0, 1 / 3, 3.4028235e38])])
    rows = [{"image_id": 7, "gt_boxes": [vals.tolist()[i:i + 4] for i in range(0, 8, 4)], "iou": vals.tolist()}]
    path = tmp_path / "layouts.json"
    path.write_text(json.dumps({"images": rows}))
    back = json.loads(path.read_text())["images"][0]
    got = np.asarray(back["iou"], dtype=np.float64).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), vals.view(np.uint32))
    assert all(_bits(a) == _bits(b) for r, s in zip(back["gt_boxes"], rows[0]["gt_boxes"]) for a, b in zip(r, s))


def _vocabs():
    from canonicalsg2im_amd.synth import make_vocab
    return make_vocab("tiny"), make_vocab("clevr")


def test_ids_to_names_to_ids_is_the_identity_over_both_vocabulary_forms():
    from canonicalsg2im_amd import authored
    flat, clevr = _vocabs()
    ids = [[i] for i in range(1, 7)]
    names = authored.object_names(ids, flat)
    assert names == ["obj_%d" % i for i in range(1, 7)]
    assert authored.object_ids(names, flat, ValueError) == ids
    rows = [[s, c, m, z] for s in range(1, 4) for c in range(1, 9) for m in range(1, 3) for z in range(1, 3)]
    named = authored.object_names(rows, clevr)
    assert named[0] == {"shape": "shape_1", "color": "color_1", "material": "material_1", "size": "size_1"}
    assert authored.object_ids(named, clevr, ValueError) == rows
    # and the other way round, through the padded tensors generate_layouts builds
    from canonicalsg2im_amd.split import layout_batch
    objs, boxes = layout_batch([(5, rows[:3], [[0.1, 0.2, 0.3, 0.4]] * 3), (6, rows[3:4], [[0.5, 0.5, 0.25, 0.25]])], clevr)
    assert tuple(objs.shape) == (2, 4, 4) and objs[0, :3].tolist() == rows[:3] and objs[1, 0].tolist() == rows[3]
    assert bool((objs[0, 3] == 0).all()) and bool((objs[1, 1:] == 0).all())                 # __image__, then padding
    assert bool((boxes[0, 3] == -1).all()) and bool((boxes[1, 1:] == -1).all())
    assert boxes.dtype == torch.float32 and boxes[1, 0].tolist() == [0.5, 0.5, 0.25, 0.25]
    with pytest.raises(ValueError, match="no objects has the id 9"):
        authored.object_names([[9]], flat)
    with pytest.raises(ValueError, match="object 0 has 1 ids"):
        authored.object_names([[1]], clevr)


def test_every_refusal_of_a_layout_row_names_its_index_and_token():
    from canonicalsg2im_amd.split import encode_layouts
    flat, clevr = _vocabs()
    box = [0.1, 0.2, 0.3, 0.4]
    good = {"image_id": 1, "objects": ["obj_1", "obj_2"], "predicted_boxes": [box, box], "gt_boxes": [box, box]}
    assert encode_layouts([good], "pred", flat) == [(1, [[1], [2]], [box, box])]

    cube = {"shape": "shape_1", "color": "color_2", "material": "material_1", "size": "size_2"}
    good4 = dict(good, objects=[cube, cube])
    assert encode_layouts([good4], "gt", clevr) == [(1, [[1, 2, 1, 2]] * 2, [box, box])]

    def row(**kw):
        return [good, dict(good, image_id=2, **kw)]

    def row4(**kw):
        return [good4, dict(good4, image_id=2, **kw)]

    for rows, which, vocab, text in (
            (row(objects=["obj_1", "zebra"]), "pred", flat, "layouts row 1: object 1: unknown objects 'zebra'"),
            (row(objects=["obj_1", "__image__"]), "pred", flat, "layouts row 1: object 1: unknown objects '__image__'"),
            (row4(objects=[dict(cube, color="mauve")], predicted_boxes=[box]), "pred", clevr, "layouts row 1: object 0: unknown color 'mauve'"),
            (row4(objects=[{"shape": "shape_1"}], predicted_boxes=[box]), "pred", clevr,
             "layouts row 1: object 0 lacks the attribute 'color'"),
            (row4(objects=["shape_1"], predicted_boxes=[box]), "pred", clevr, "layouts row 1: object 0 is the name 'shape_1'"),
            ([good, {k: v for k, v in good.items() if k != "gt_boxes"} | {"image_id": 2}], "gt", flat,
             "layouts row 1: no 'gt_boxes'"),
            (row(predicted_boxes=[box]), "pred", flat, "layouts row 1: 2 objects but 1 predicted_boxes"),
            (row(predicted_boxes=[box, [0.1, 0.2, 0.3]]), "pred", flat, r"layouts row 1: predicted_boxes\[1\] = \[0.1, 0.2, 0.3\]"),
            (row(gt_boxes=[[0.1, float("nan"), 0.3, 0.4], box]), "gt", flat, r"layouts row 1: gt_boxes\[0\] = \[0.1, nan, 0.3, 0.4\]"),
            (row(gt_boxes=[box, [0.1, float("inf"), 0.3, 0.4]]), "gt", flat, r"layouts row 1: gt_boxes\[1\] = .*inf.*four finite"),
            (row(predicted_boxes=[box, [0.1, "0.2", 0.3, 0.4]]), "pred", flat, r"layouts row 1: predicted_boxes\[1\] = .*'0.2'"),
            ([good, dict(good)], "pred", flat, "layouts row 1: image_id 1 a second time"),
            ([good, "a string"], "pred", flat, "layouts row 1: a row is .*'a string'"),
            ([good, dict(good, image_id=None)], "pred", flat, "layouts row 1: image_id None"),
    ):
        with pytest.raises(ValueError, match=text):
            encode_layouts(rows, which, vocab)
    with pytest.raises(ValueError, match="which must be 'pred' or 'gt', got 'both'"):
        encode_layouts([good], "both", flat)
    with pytest.raises(ValueError, match="non-empty list"):
        encode_layouts([], "pred", flat)

    class Refuses:                                          # generate_layouts checks every row before it touches the sampler
        class opt:
            vocab = flat
            batch_size = 2

        @property
        def device(self):
            raise AssertionError("the sampler was touched before the rows were checked")

    from canonicalsg2im_amd.split import generate_layouts
    with pytest.raises(ValueError, match="layouts row 1: object 1: unknown objects 'zebra'"):
        generate_layouts(Refuses(), row(objects=["obj_1", "zebra"]), "pred", deprocess="imagenet")
    with pytest.raises(ValueError, match="'imagenet' or 'decode_img'.*'srgb'"):
        generate_layouts(Refuses(), [good], "pred", deprocess="srgb")


def test_a_duplicate_image_id_is_refused_before_the_sample_is_written(tmp_path):
    """The host half of one batch as generate_split hands it over: the third sample repeats the first's id."""
    from PIL import Image

    from canonicalsg2im_amd import split
    flat, _ = _vocabs()
    pics = _pictures(6)
    boxes = np.full((3, 3, 4), -1, np.float32)
    boxes[:, :2] = np.float32([0.1, 0.2, 0.3, 0.4])
    host = {"image_id": np.asarray([4, 5, 4]), "objs": np.asarray([[[1], [2], [0]]] * 3), "boxes": boxes,
            "gt": pics[:3], "generation/gt_box_gt_mask": pics[3:]}
    files = split.FileWriter(2, "png")
    taker = split.SplitRows(flat, files, split._Paths(str(tmp_path), "png"))
    with pytest.raises(ValueError, match="image id 4 a second time in one run: it would overwrite a file"):
        taker.take(host)
    files.close()
    assert [r["image_id"] for r in taker.rows] == [4, 5]
    assert taker.rows[0]["objects"] == ["obj_1", "obj_2"] and "predicted_boxes" not in taker.rows[0]     # no graph part
    assert np.array_equal(np.float32(taker.rows[1]["gt_boxes"]), boxes[1, :2])
    assert sorted(os.listdir(tmp_path / "gt")) == ["4.png", "5.png"] == sorted(os.listdir(tmp_path / "generation" / "gt_box_gt_mask"))
    first = np.asarray(Image.open(tmp_path / "gt" / "4.png")).transpose(2, 0, 1)
    assert np.array_equal(first, pics[0])                   # the first sample's picture, not the repeated id's
    box = [0.1, 0.2, 0.3, 0.4]
    with pytest.raises(ValueError, match="layouts row 2: image_id 4 a second time: it would overwrite a file"):
        split.encode_layouts([{"image_id": 4, "objects": ["obj_1"], "gt_boxes": [box]},
                              {"image_id": 5, "objects": ["obj_1"], "gt_boxes": [box]},
                              {"image_id": 4, "objects": ["obj_1"], "gt_boxes": [box]}], "gt", flat)


# ------------------------------------------------------------------------------------------------- 3. the command line
@pytest.fixture()
def ckpt(tmp_path):
    path = tmp_path / "weights.pt"
    path.write_bytes(b"not read: every refusal below comes first")
    return str(path)


def test_the_three_flags_exclude_each_other(tmp_path, ckpt):
    from canonicalsg2im_amd.scripts import sample as cli
    other = tmp_path / "rows.json"
    other.write_text("[]")
    for flags, text in (
            (["--split", "val", "--layouts", str(other)], "--split and --layouts exclude each other"),
            (["--split", "train", "--scene_graphs", str(other)], "--split and --scene_graphs exclude each other"),
            (["--layouts", str(other), "--scene_graphs", str(other)], "--layouts and --scene_graphs exclude each other"),
            (["--split", "val", "--layouts", str(other), "--scene_graphs", str(other)],
             "--split and --layouts and --scene_graphs exclude each other")):
        with pytest.raises(SystemExit, match=text):
            cli.parse_args(flags + ["--checkpoint_name", ckpt, "--output_dir", str(tmp_path / "out")])
    with pytest.raises(SystemExit, match="--split needs --checkpoint_name"):
        cli.parse_args(["--split", "val"])
    with pytest.raises(SystemExit, match="--layouts needs --checkpoint_name"):
        cli.parse_args(["--layouts", str(other), "--output_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--layouts needs --output_dir"):
        cli.parse_args(["--layouts", str(other), "--checkpoint_name", ckpt])
    with pytest.raises(SystemExit, match="--layouts .*nowhere.json: no such file"):
        cli.parse_args(["--layouts", str(tmp_path / "nowhere.json"), "--checkpoint_name", ckpt, "--output_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--img_deprocess srgb: --split draws through decode_img or imagenet"):
        cli.parse_args(["--split", "val", "--checkpoint_name", ckpt, "--img_deprocess", "srgb"])
    with pytest.raises(SystemExit, match="--num_writers within 1 .. 16"):
        cli.parse_args(["--split", "val", "--checkpoint_name", ckpt, "--num_writers", "17"])
    with pytest.raises(SystemExit):                         # argparse's own: not a split
        cli.parse_args(["--split", "test", "--checkpoint_name", ckpt])
    args = cli.parse_args(["--split", "val", "--checkpoint_name", ckpt])
    assert (args.max_pictures, args.image_format, args.num_writers, args.layout_boxes, args.img_deprocess) == \
        (0, "png", 8, "pred", "decode_img")
    plain = cli.parse_args([])                              # the two existing modes: untouched
    assert plain.split is None and plain.layouts is None and plain.scene_graphs is None


@pytest.mark.parametrize("dataset, where", [
    ("coco", os.path.join("MSCoco", "images", "val2017")), ("packed_coco", os.path.join("MSCoco", "images", "val2017")),
    ("packed_clevr", os.path.join("CLEVR", "CLEVR_Dialog", "images", "val")), ("packed_vg", os.path.join("vg", "images"))])
def test_a_missing_folder_ends_the_run_with_its_directory_before_any_device_call(tmp_path, ckpt, monkeypatch, dataset, where):
    from canonicalsg2im_amd.scripts import sample as cli
    root = str(tmp_path / "nowhere")

    def no_device(*a, **k):
        raise AssertionError("a device call came before the folder check")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(SystemExit) as e:
        cli.main(["--split", "val", "--checkpoint_name", ckpt, "--dataset", dataset, "--dataroot", root])
    assert os.path.join(root, where) in str(e.value) and "no synthetic stand-in" in str(e.value), str(e.value)
