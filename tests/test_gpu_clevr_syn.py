"""`--dataset packed_clevr_syn` on a real MI355X: the device batch against the reference's `__getitem__` + collate
(tests/golden/clevr_syn.npz, part b), and the large-graph run end to end on a 64 x 64 random-weight model.  No tolerance:
ids, graphs and counts are integers and the boxes are compared by their bits."""
import argparse
import json
import os

import pytest
import torch

from conftest import load_golden
from test_gpu_split import _checkpoint

pytestmark = pytest.mark.gpu

MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--no_vgg_loss", "--use_img_disc", "1", "--gconv_hidden_dim", "64",
         "--gconv_dim", "32", "--dataset", "packed_clevr_syn"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("lt", [0, 1])
def test_device_batch_equals_the_reference_collate(cuda, lt):
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    meta, z = load_golden("clevr_syn")
    rows = 0
    for run in meta["runs"]:
        if run.get("getitem"):
            continue
        ds = syn.SynClevrScenes(run["min_objects"], run["max_objects"], run["max_samples"], run["seed"])
        args = argparse.Namespace(dataset="packed_clevr_syn", vocab=ds.vocab, learned_transitivity=lt, learned_converse=0)
        source = syn.SynClevrBatches(ds, args, None, cuda)
        (batch,) = list(source.batches([list(range(len(ds)))]))
        imgs, objs, boxes, triplets, _, ttype, masks, ids = batch
        torch.cuda.synchronize()
        pre = "%s_lt%d_" % (run["key"], lt)
        assert imgs is None and masks is None and ids.dtype == torch.int64 and ids.cpu().tolist() == list(range(len(ds)))
        assert objs.is_cuda and boxes.is_cuda and triplets.is_cuda and boxes.dtype == torch.float32
        assert torch.equal(objs.cpu(), z[pre + "objs"].to(torch.int64))
        assert torch.equal(boxes.cpu().view(torch.int32), z[pre + "boxes"].view(torch.int32))
        assert torch.equal(triplets.cpu(), z[pre + "triplets"].to(torch.int64))
        assert torch.equal(ttype.cpu(), z[pre + "triplet_type"].to(torch.int64))
        assert torch.equal(batch.objs_host, objs.cpu())
        rows += int(triplets.shape[0] * triplets.shape[1])
    assert rows > (5000 if lt else 500)


@pytest.mark.timeout(120)
def test_scenes_of_one_object_get_their_dummy_alone(cuda):
    """The reference's own __getitem__ raises on such a scene (it indexes the empty array of location triplets); the
    graph it was about to make is the `__in_image__` dummy, and that is what the batch holds."""
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    ds = syn.SynClevrScenes(1, 1, 3, 0)
    args = argparse.Namespace(dataset="packed_clevr_syn", vocab=ds.vocab, learned_transitivity=1, learned_converse=0)
    (batch,) = list(syn.SynClevrBatches(ds, args, None, cuda).batches([[0, 1, 2]]))
    _, objs, boxes, triplets, _, ttype, _, ids = batch
    in_image = ds.vocab["pred_name_to_idx"]["__in_image__"]
    assert tuple(objs.shape) == (3, 2, 4) and bool((objs[:, 0] > 0).all()) and bool((objs[:, 1] == 0).all())
    assert bool((boxes[:, 1] == -1).all()) and bool((boxes[:, 0, 2:] > 0).all())
    assert triplets.cpu().tolist() == [[[0, in_image, 1]]] * 3 and ttype.cpu().tolist() == [[0]] * 3


@pytest.fixture(scope="module")
def run(cuda, tmp_path_factory):
    """The run once: two batches of 3 scenes of 3 to 6 objects through scripts.sample; shared, left unchanged."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts import sample
    from canonicalsg2im_amd.sg2im.data.packed_clevr import clevr_vocab
    root = tmp_path_factory.mktemp("clevr_syn_run")
    out, scenes, ckpt_path = str(root / "out"), str(root / "scenes.json"), str(root / "itr_3.pt")
    opt = T.make_opt(clevr_vocab(), MODEL + ["--batch_size", "3"])
    _, ckpt = _checkpoint(opt, cuda)
    torch.save(ckpt, ckpt_path)
    argv = MODEL + ["--batch_size", "3", "--min_objects", "3", "--max_objects", "6", "--max_samples", "6", "--seed", "4",
                    "--scenes", scenes, "--checkpoint_name", ckpt_path, "--output_dir", out]
    sample.main(argv)
    return {"out": out, "scenes": scenes, "ckpt_path": ckpt_path, "ckpt": ckpt, "opt": opt, "argv": argv}


@pytest.mark.timeout(300)
def test_the_run_writes_its_files_and_the_report_adds_up(run):
    out = run["out"]
    found = sorted(os.path.relpath(os.path.join(d, n), out).replace(os.sep, "/") for d, _, names in os.walk(out) for n in names)
    assert found == sorted(["layouts.json", "generalisation.json"] +
                           ["generation/%s/%d.png" % (s, i) for s in ("gt_box_gt_mask", "pred_box_pred_mask") for i in range(6)])
    doc = json.load(open(os.path.join(out, "generalisation.json")))
    assert set(doc) == {"dataset", "checkpoint", "seed", "scenes", "min_objects", "max_objects", "images", "metrics",
                        "relation_agreement", "by_num_objects"}
    assert doc["dataset"] == "packed_clevr_syn" and doc["seed"] == 4 and doc["scenes"] == run["scenes"] and doc["images"] == 6
    assert doc["checkpoint"] == run["ckpt_path"] and 3 <= doc["min_objects"] <= doc["max_objects"] <= 6
    assert set(doc["metrics"]) == {"avg_iou", "total_iou_05", "total_iou_03", "num_boxes"}
    rel = doc["relation_agreement"]
    assert set(rel) == {"agreeing", "tested", "rate", "by_type", "by_predicate"}
    assert set(rel["by_type"]) == {"original", "transitive", "symmetric", "anti_symmetric"}
    assert 0 <= rel["agreeing"] <= rel["tested"] and rel["tested"] > 0 and rel["by_type"]["original"]["tested"] == rel["tested"]
    assert set(rel["by_predicate"]) <= {"__below__", "__above__", "__left of__", "__right of__", "__inside__", "__surrounding__"}
    assert sum(v["tested"] for v in rel["by_predicate"].values()) == rel["tested"]
    assert sum(v["agreeing"] for v in rel["by_predicate"].values()) == rel["agreeing"]
    by = doc["by_num_objects"]
    layouts = json.load(open(os.path.join(out, "layouts.json")))
    sizes = [len(r["objects"]) for r in layouts["images"]]
    assert sorted(by, key=int) == [str(n) for n in sorted(set(sizes))] and all(3 <= n <= 6 for n in sizes)
    assert sum(v["images"] for v in by.values()) == 6 and sum(v["num_boxes"] for v in by.values()) == doc["metrics"]["num_boxes"]
    assert sum(v["relation_agreement"]["tested"] for v in by.values()) == rel["tested"]
    assert sum(v["relation_agreement"]["agreeing"] for v in by.values()) == rel["agreeing"]
    for k in ("original", "transitive", "symmetric", "anti_symmetric"):
        assert sum(v["relation_agreement"]["by_type"][k]["tested"] for v in by.values()) == rel["by_type"][k]["tested"]
    assert layouts["dataset"] == "packed_clevr_syn" and layouts["split"] == "synthetic"
    assert layouts["metrics"]["relation_agreement"] == rel and [r["image_id"] for r in layouts["images"]] == list(range(6))
    # the scenes file was written, and a second dataset reads the same scenes from it
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    assert syn.SynClevrScenes(scenes_json=run["scenes"]).scenes == syn.SynClevrScenes(3, 6, 6, 4).scenes


@pytest.mark.timeout(300)
def test_generate_split_without_relations_is_unchanged_key_for_key(run, cuda):
    """relations=False (the default): the metrics, the rows and layouts.json hold the keys they held before the parameter
    existed, and their values are those of the relations=True walk, bit for bit."""
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.scripts.train import folder_builder
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    from canonicalsg2im_amd.sg2im.data.loader import file_order_batches
    from canonicalsg2im_amd.split import generate_split
    ds = syn.SynClevrScenes(scenes_json=run["scenes"])
    walks = []
    for kw in ({}, {"relations": False}, {"relations": True}):
        torch.manual_seed(0)
        sampler = Sampler(run["opt"], cuda, run["ckpt"])
        builder = folder_builder(ds, run["opt"], sampler, cuda)
        walks.append(generate_split(sampler, builder.batches(file_order_batches(len(ds), 3)), None, deprocess="decode_img", **kw))
    (m0, r0), (m1, r1), (m2, r2) = walks
    assert set(m0) == {"avg_iou", "total_iou_05", "total_iou_03", "num_boxes"} and m0 == m1
    assert all(set(r) == {"image_id", "objects", "gt_boxes", "predicted_boxes", "iou"} for r in r0) and r0 == r1
    assert set(m2) == set(m0) | {"relation_agreement"} and {k: m2[k] for k in m0} == m0
    assert all(set(r) == set(r0[0]) | {"relation_agreement"} for r in r2)
    assert [{k: v for k, v in r.items() if k != "relation_agreement"} for r in r2] == r0
    doc = json.load(open(os.path.join(run["out"], "generalisation.json")))
    assert m2["relation_agreement"] == doc["relation_agreement"] and {k: m2[k] for k in m0} == doc["metrics"]
