"""The host half of `--dataset packed_clevr_syn` (canonicalsg2im_amd/sg2im/data/packed_clevr_syn.py): the drawn scenes
against the reference's (tests/golden/clevr_syn.npz, part a), the scenes file, the refusals, the centres, and the host
arithmetic of generalisation.json.  CPU only; every comparison is exact."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    meta, z = load_golden("clevr_syn")
    return meta, {k: v.numpy() for k, v in z.items()}


def _syn():
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn
    return packed_clevr_syn


def test_drawn_scenes_equal_the_reference_value_for_value(golden):
    syn = _syn()
    meta, z = golden
    assert meta["attributes"] == list(syn.ATTRIBUTES)
    objects = 0
    for run in meta["runs"]:
        ds = syn.SynClevrScenes(run["min_objects"], run["max_objects"], run["max_samples"], run["seed"])
        counts = z[run["key"] + "_counts"]
        assert len(ds) == run["max_samples"] and [len(s["objects"]) for s in ds.scenes] == counts.tolist()
        assert [s["image_index"] for s in ds.scenes] == [str(j) for j in range(len(ds))] and ds.image_ids == list(range(len(ds)))
        for b, n in enumerate(counts):
            objs, boxes, _ = ds.annotations(b)
            assert objs.dtype == np.int64 and boxes.dtype == np.float64
            assert np.array_equal(objs, z[run["key"] + "_ids"][b, :n])
            assert np.array_equal(boxes.view(np.int64), z[run["key"] + "_boxes64"][b, :n].view(np.int64))     # fp64 bits
            objects += int(n)
    assert objects > 150
    assert syn.SynClevrScenes(3, 3, 2, 0).scenes != syn.SynClevrScenes(3, 3, 2, 1).scenes
    assert syn.SynClevrScenes().vocab == __import__("canonicalsg2im_amd.sg2im.data.packed_clevr", fromlist=["x"]).clevr_vocab()


def test_scenes_file_round_trip(tmp_path):
    syn = _syn()
    path = str(tmp_path / "scenes.json")
    first = syn.SynClevrScenes(2, 6, 7, seed=3, scenes_json=path)
    assert not first.loaded and os.path.isfile(path)
    again = syn.SynClevrScenes(9, 9, 1, seed=8, scenes_json=path)        # the file wins over the four numbers
    assert again.loaded and again.seed == 3 and len(again) == 7
    for i in range(7):
        for a, b in zip(first.annotations(i), again.annotations(i)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert json.load(open(path))["scenes"] == first.scenes            # plain JSON, nothing else in it
    for text, what in (("[]", "non-empty list"), ('[{"image_index": "0", "objects": [], "boxes": []}]', "0 objects"),
                       ('[{"image_index": "0", "objects": [{"shape": "cone", "color": "red", "material": "metal", "size": '
                        '"small"}], "boxes": [[0, 0, 0.1, 0.1]]}]', "has no shape"),
                       ('[{"image_index": "0", "objects": [{"shape": "cube", "color": "red", "material": "metal", "size": '
                        '"small"}], "boxes": [[0, 0, 0.1]]}]', "four finite numbers")):
        bad = str(tmp_path / "bad.json")
        open(bad, "w").write(text)
        with pytest.raises(ValueError, match=what):
            syn.SynClevrScenes(scenes_json=bad)


def test_refusals_when_the_dataset_is_made():
    syn = _syn()
    with pytest.raises(ValueError, match="max_objects must be at most 255 .got 256."):
        syn.SynClevrScenes(15, 256, 1, 0)
    with pytest.raises(ValueError, match="min_objects must be at least 1 .got 0."):
        syn.SynClevrScenes(0, 3, 1, 0)
    with pytest.raises(NotImplementedError, match="mask_size must be 0 .got 16."):
        syn.SynClevrScenes(3, 3, 1, 0, mask_size=16)
    with pytest.raises(ValueError, match="below min_objects"):
        syn.SynClevrScenes(5, 3, 1, 0)
    assert len(syn.SynClevrScenes(255, 255, 1, 0).scenes[0]["objects"]) == 255


def test_registered_where_the_folder_datasets_dispatch():
    from canonicalsg2im_amd.scripts import sample, train
    from canonicalsg2im_amd.sg2im.data import FOLDER_DATASETS, build_folder_dataset, looked_for
    assert FOLDER_DATASETS["packed_clevr_syn"] == ("packed_clevr_syn", "build_clevr_syn_dataset")
    args = sample.build_parser().parse_args(["--dataset", "packed_clevr_syn", "--min_objects", "2", "--max_objects", "4",
                                             "--max_samples", "5", "--seed", "1"])
    ds = build_folder_dataset(args, "val")
    assert len(ds) == 5 and ds.seed == 1 and all(2 <= len(s["objects"]) <= 4 for s in ds.scenes)
    assert ds.scenes == _syn().SynClevrScenes(2, 4, 5, 1).scenes and "no folder" in looked_for(args, "val")
    args.mask_size = 8
    with pytest.raises(NotImplementedError, match="mask_size must be 0"):
        build_folder_dataset(args, "val")
    with pytest.raises(SystemExit, match="cannot be trained on: its samples carry no picture"):
        train.main(["--dataset", "packed_clevr_syn"])
    # scripts.sample: generate_clevr.py's defaults, and what the run needs
    with pytest.raises(SystemExit, match="needs --checkpoint_name and --output_dir"):
        sample.parse_args(["--dataset", "packed_clevr_syn"])
    ckpt = os.path.abspath(__file__)                       # any file that exists: parse_args only looks for it
    a = sample.parse_args(["--dataset", "packed_clevr_syn", "--checkpoint_name", ckpt, "--output_dir", "out"])
    assert (a.min_objects, a.max_objects, a.max_samples, a.batch_size, a.seed, a.scenes, a.inception_weights) == \
        (15, 30, 1000, 10, 0, None, None)
    with pytest.raises(SystemExit, match="--split does not go with it"):
        sample.parse_args(["--dataset", "packed_clevr_syn", "--checkpoint_name", ckpt, "--output_dir", "out", "--split", "val"])
    assert sample.build_parser().parse_args([]).batch_size == 4          # every other dataset keeps the parser's default


def test_centres_are_rounded_from_fp64_not_formed_from_the_fp32_boxes(golden):
    syn = _syn()
    meta, z = golden
    differing = total = 0
    for run in meta["runs"]:
        if run.get("getitem"):
            continue
        ds = syn.SynClevrScenes(run["min_objects"], run["max_objects"], run["max_samples"], run["seed"])
        source = syn.SynClevrBatches(ds, argparse.Namespace(), None, torch.device("cpu"))
        objs, boxes, centres, counts, ids = source.host_batch(list(range(len(ds))))
        want = z[run["key"] + "_lt0_centers"]                 # what the reference's __getitem__ hands to its pair rule
        for b, n in enumerate(counts.tolist()):
            assert torch.equal(centres[b, :n].view(torch.int32), torch.from_numpy(want[b, :n].copy()).view(torch.int32))
            assert torch.equal(boxes[b, :n].view(torch.int32),
                               torch.from_numpy(z[run["key"] + "_lt0_boxes"][b, :n].copy()).view(torch.int32))
            assert bool((boxes[b, n:] == -1).all()) and bool((objs[b, n:] == 0).all())
            from_boxes = boxes[b, :n, :2] + 0.5 * boxes[b, :n, 2:]                      # fp32: the other way to form them
            differing += int((from_boxes != centres[b, :n]).sum())
            total += 2 * n
        assert objs.dtype == torch.int64 and boxes.dtype == torch.float32 and centres.dtype == torch.float32
        assert ids.tolist() == list(range(len(ds))) and ids.dtype == torch.int64
    print("centres: %d of %d recorded values differ from the fp32 boxes' centres" % (differing, total))
    assert differing >= 1


def _row(n, iou, agreeing, tested):
    return {"image_id": 0, "objects": ["cube"] * n, "gt_boxes": [[0, 0, 1, 1]] * n, "predicted_boxes": [[0, 0, 1, 1]] * n,
            "iou": iou, "relation_agreement": {"agreeing": agreeing, "tested": tested}}


def test_generalisation_report_sums_the_rows_by_graph_size():
    from canonicalsg2im_amd import split
    from canonicalsg2im_amd.sg2im.data.packed_clevr import clevr_vocab
    vocab = clevr_vocab()
    totals = [[[0, 0] for _ in range(8)] for _ in range(4)]
    totals[0][2], totals[0][5], totals[1][5] = [3, 4], [1, 2], [2, 6]
    summary = split.relation_summary(totals, vocab)
    assert summary["agreeing"] == 6 and summary["tested"] == 12 and summary["rate"] == 0.5
    assert summary["by_type"]["original"] == {"agreeing": 4, "tested": 6, "rate": 4 / 6}
    assert summary["by_type"]["symmetric"] == {"agreeing": 0, "tested": 0, "rate": None}
    assert summary["by_predicate"] == {"__below__": {"agreeing": 3, "tested": 4, "rate": 0.75},
                                       "__right of__": {"agreeing": 3, "tested": 8, "rate": 3 / 8}}
    rows = [_row(2, [0.5, 0.75], [1, 1, 0, 0], [2, 3, 0, 0]), _row(3, [0.25, 0.0, 1.0], [2, 1, 0, 0], [3, 3, 0, 0]),
            _row(2, [0.125, 0.375], [1, 0, 0, 0], [1, 0, 0, 0])]
    metrics = {"avg_iou": 3.0 / 7, "total_iou_05": 2 / 7, "total_iou_03": 3 / 7, "num_boxes": 7.0, "relation_agreement": summary}
    doc = split.generalisation_report(metrics, rows, seed=0, scenes=None, checkpoint="itr_1.pt")
    assert set(doc) == {"seed", "scenes", "checkpoint", "images", "metrics", "relation_agreement", "by_num_objects"}
    assert doc["metrics"] == {k: v for k, v in metrics.items() if k != "relation_agreement"} and doc["images"] == 3
    by = doc["by_num_objects"]
    assert list(by) == ["2", "3"] and by["2"]["images"] == 2 and by["2"]["num_boxes"] == 4 and by["3"]["num_boxes"] == 3
    assert by["2"]["avg_iou"] == (0.5 + 0.75 + 0.125 + 0.375) / 4 and by["2"]["total_iou_05"] == 0.25 and by["2"]["total_iou_03"] == 0.75
    assert by["2"]["relation_agreement"]["by_type"]["original"] == {"agreeing": 2, "tested": 3, "rate": 2 / 3}
    assert sum(v["relation_agreement"]["tested"] for v in by.values()) == summary["tested"]
    assert sum(v["relation_agreement"]["agreeing"] for v in by.values()) == summary["agreeing"]
    assert sum(v["num_boxes"] for v in by.values()) == metrics["num_boxes"]
    json.dumps(doc)
