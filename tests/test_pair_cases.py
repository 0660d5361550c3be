"""The sampled-pair graph of the unpacked `coco` dataset on the CPU: tests/pair_cases.py's restatements against what the
reference itself made (tests/golden/coco_pairs.npz), the comparison rule csg_pair_relations decides by against the
reference's math.atan2 inequalities, the host draws against the reference's recorded random stream, and the dataset's
filtering against packed_coco's."""
import json
import os
import random
import types

import numpy as np
import pytest

import pair_cases as pc


# ------------------------------------------------------------------------------------------------- 1. the restatements
@pytest.mark.parametrize("case", pc.cases(), ids=pc.case_id)
def test_restatement_reproduces_the_reference_rows_and_graph(case):
    s, group, g = pc.case_arrays(*case)
    vocab = pc.vocab()
    p2i = vocab["pred_name_to_idx"]
    B, O = g["other"].shape
    assert g["objs"].shape == (B, O + 1) and g["boxes"].dtype == np.float32 and O == g["n"].max()
    centers = pc.centers_of(g["boxes"])
    rows = [pc.pair_rows_atan2(g["boxes"][b], centers[b], int(g["n"][b]), g["other"][b], g["flip"][b], p2i,
                               use_converse=bool(s["use_converse"])) for b in range(B)]
    for b in range(B):
        drawn = int(g["n"][b]) if s["include_relationships"] and g["n"][b] >= 2 else 0
        assert len(rows[b]) == drawn and (g["other"][b, :drawn] >= 0).all() and (g["other"][b, drawn:] == -1).all()
        assert int(g["objs"][b, g["n"][b]]) == 0 and (g["objs"][b, :g["n"][b]] > 0).all()      # __image__ follows the objects
    assert np.array_equal(pc.padded_rows(rows, O, p2i), g["rows"])
    kw = {}
    if s["learned_converse"]:
        kw = {"learned_converse": True, "converse_weights": g["weights"],
              "uniforms": pc.golden_uniforms(group, group["converse_draws"])}
    trip, ttype, conv = pc.batch_from_rows(g["rows"], g["n"], vocab, learned_transitivity=bool(s["learned_transitivity"]), **kw)
    assert list(trip.shape) == group["triplets"]
    assert np.array_equal(trip, g["triplets"]) and np.array_equal(ttype, g["tt"]) and np.array_equal(conv, g["conv"])
    assert int(conv.sum()) == group["converse_draws"]


def test_the_golden_file_meets_every_tie_and_every_predicate():
    meta, _ = pc.golden()
    names = pc.vocab()["pred_idx_to_name"]
    ties, preds, corner_only = set(), set(), 0
    for case in pc.cases():
        s, _, g = pc.case_arrays(*case)
        centers = pc.centers_of(g["boxes"])
        for b in range(g["other"].shape[0]):
            for cur in range(int((g["other"][b] >= 0).sum())):
                j = int(g["other"][b, cur])
                so = (j, cur) if g["flip"][b, cur] else (cur, j)
                d = centers[b, so[0]] - centers[b, so[1]]
                if abs(d[0]) == abs(d[1]) or d[0] == 0 or d[1] == 0:
                    ties.add((int(np.sign(d[0])), int(np.sign(d[1]))))
                preds.add(names[g["rows"][b, cur, 1]])
                bs, bo = g["boxes"][b, so[0]], g["boxes"][b, so[1]]
                corners = bs[0] < bo[0] and bs[1] < bo[1] and bs[0] + bs[2] > bo[0] + bo[2] and bs[1] + bs[3] > bo[1] + bo[3]
                corner_only += bool(corners and names[g["rows"][b, cur, 1]] != "__surrounding__" and not s["use_converse"])
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0), (0, -1), (-1, 0)} <= ties
    assert preds == {"__surrounding__", "__inside__", "__left of__", "__right of__", "__above__", "__below__"}
    assert corner_only >= 1
    assert sorted(set(pc.golden()[1]["counts"].tolist())) == [1, 2, 3, 5, 8]
    assert [(s["use_converse"], s["learned_transitivity"], s["include_relationships"], s["learned_converse"])
            for s in meta["settings"]] == [(0, 0, 1, 0), (1, 0, 1, 0), (0, 1, 1, 0), (1, 1, 1, 0), (0, 0, 0, 0), (0, 1, 1, 1)]


# ------------------------------------------------------------------------------------------------- 2. the sector rule
def test_comparison_rule_equals_the_atan2_rule():
    pairs = pc.tie_pairs()
    for case in pc.cases():                                    # the table: every difference the golden samples can form
        _, _, g = pc.case_arrays(*case)
        centers = pc.centers_of(g["boxes"])
        for b in range(centers.shape[0]):
            n = int(g["n"][b])
            pairs += [tuple(centers[b, i] - centers[b, j]) for i in range(n) for j in range(n) if i != j]
    for boxes, _ in pc.hand_written():
        c = pc.centers_of(boxes)
        pairs += [tuple(c[0] - c[1]), tuple(c[1] - c[0])]
    exact_ties = sum(1 for dx, dy in pairs if abs(dx) == abs(dy))
    mismatches = [(dx, dy) for dx, dy in pairs if pc.sector_by_comparison(dx, dy) != pc.sector_by_atan2(dx, dy)]
    print("%d fp32 pairs, %d exact ties, %d mismatches" % (len(pairs), exact_ties, len(mismatches)))
    assert len(pairs) > 4000 and exact_ties > 200 and not mismatches, mismatches[:5]
    z, a = np.float32(0.0), np.float32(0.25)
    assert pc.sector_by_comparison(z, z) == pc.RIGHT and pc.sector_by_comparison(-z, z) == pc.LEFT     # atan2(0, -0) = pi
    assert pc.sector_by_comparison(-z, -z) == pc.LEFT and pc.sector_by_comparison(z, -z) == pc.RIGHT
    assert [pc.sector_by_comparison(*d) for d in ((a, a), (a, -a), (-a, a), (-a, -a), (z, -a), (-a, z), (z, a))] == \
        [pc.BELOW, pc.RIGHT, pc.LEFT, pc.LEFT, pc.ABOVE, pc.LEFT, pc.BELOW]


# ------------------------------------------------------------------------------------------------- 3. the draws
def _stub_builder(counts, include_relationships, rng):
    from canonicalsg2im_amd.sg2im.data.coco import CocoPairsBatchBuilder
    ds = types.SimpleNamespace(num_objects=lambda i: int(counts[i]), include_relationships=bool(include_relationships))
    b = CocoPairsBatchBuilder(ds, None, None, None, rng=rng)
    b.close()
    return b


@pytest.mark.parametrize("case", pc.cases(), ids=pc.case_id)
def test_replaying_the_seed_through_draw_gives_the_reference_pairs(case):
    s, group, g = pc.case_arrays(*case)
    counts = pc.golden()[1]["counts"]
    builder = _stub_builder(counts, s["include_relationships"], random.Random(group["seed"]))
    drawn = builder.draw(group["samples"])
    B, O = g["other"].shape
    other, flip = np.full((B, O), -1, np.int32), np.zeros((B, O), np.uint8)
    for b, pairs in enumerate(drawn):
        assert len(pairs) in (0, int(counts[group["samples"][b]]))
        for cur, (j, f) in enumerate(pairs):
            other[b, cur], flip[b, cur] = j, f
    assert np.array_equal(other, g["other"]) and np.array_equal(flip, g["flip"])
    if not s["include_relationships"]:
        assert builder.rng.getstate() == random.Random(group["seed"]).getstate()          # nothing was drawn


def test_draw_refuses_a_batch_without_objects_and_draws_nothing_for_one_object():
    rng = random.Random(1)
    builder = _stub_builder([0, 0, 1], True, rng)
    with pytest.raises(ValueError, match="a batch of samples without objects"):
        builder.draw([0, 1])
    assert builder.draw([0, 2]) == [[], []] and rng.getstate() == random.Random(1).getstate()


# ------------------------------------------------------------------------------------------------- 4. the dataset
def _annotation_pair(tmp_path):
    """Five images: 1 has 4 objects (one too small, one 'other'), 2 has 2, 3 has no stuff annotation, 4 has 9, 5 has 3."""
    images = [{"id": i, "file_name": "%d.png" % i, "width": 100, "height": 50} for i in (1, 2, 3, 4, 5)]
    inst_cats = [{"id": 1, "name": "person"}, {"id": 3, "name": "car"}]
    stuff_cats = [{"id": 92, "name": "banner"}, {"id": 183, "name": "other"}]
    box = [10.0, 10.0, 40.0, 20.0]

    def rows(image_id, cats, first):
        return [{"id": first + k, "image_id": image_id, "category_id": c, "bbox": box, "segmentation": []}
                for k, c in enumerate(cats)]

    inst = rows(1, [1, 3], 100) + [{"id": 199, "image_id": 1, "category_id": 1, "bbox": [0.0, 0.0, 5.0, 5.0]}] + \
        rows(2, [1], 200) + rows(3, [1, 3, 1], 300) + rows(4, [1] * 8, 400) + rows(5, [3, 3], 500)
    stuff = rows(1, [92, 183], 150) + rows(2, [92], 250) + rows(4, [92], 450) + rows(5, [92], 550)
    paths = []
    for name, cats, ann in (("instances", inst_cats, inst), ("stuff", stuff_cats, stuff)):
        paths.append(str(tmp_path / (name + ".json")))
        with open(paths[-1], "w") as f:
            json.dump({"images": images, "categories": cats, "annotations": ann}, f)
    return paths


def test_filtering_and_vocabulary_equal_packed_coco_at_the_same_limits(tmp_path):
    from canonicalsg2im_amd.sg2im.data.coco import COCO_MAX_OBJECTS, COCO_MIN_OBJECTS, CocoPairsBatchBuilder, CocoSceneGraphDataset
    from canonicalsg2im_amd.sg2im.data.packed_coco import CocoBatchBuilder, PackedCocoSceneGraphDataset
    inst, stuff = _annotation_pair(tmp_path)
    for lo, hi, want in ((1, 1000, [1, 2, 4, 5]), (3, 8, [1, 5]), (2, 3, [1, 2, 5]), (9, 9, [4]), (16, 1000, [])):
        ours = CocoSceneGraphDataset("nowhere", inst, stuff, min_objects=lo, max_objects=hi)
        packed = PackedCocoSceneGraphDataset("nowhere", inst, stuff, min_objects=lo, max_objects=hi)
        assert ours.image_ids == packed.image_ids == want and len(ours) == len(packed)
        assert ours.vocab == packed.vocab and ours.image_id_to_objects == packed.image_id_to_objects
    assert (COCO_MIN_OBJECTS, COCO_MAX_OBJECTS) == (3, 8)
    assert CocoSceneGraphDataset("nowhere", inst, stuff).image_ids == [1, 5]                  # the reference's 3 .. 8
    assert PackedCocoSceneGraphDataset("nowhere", inst, stuff).image_ids == []                # packed_coco's 16 .. 1000, as before
    assert CocoSceneGraphDataset.builder_class is CocoPairsBatchBuilder and PackedCocoSceneGraphDataset.builder_class is CocoBatchBuilder
    assert CocoPairsBatchBuilder.takes_rng and not CocoPairsBatchBuilder.keep_rgba and CocoPairsBatchBuilder.mean is None
    ours = CocoSceneGraphDataset("nowhere", inst, stuff, min_objects=1, keep_image_ids=[5, 2, 77])
    assert ours.image_ids == [2, 5] and [ours.num_objects(i) for i in range(2)] == [2, 3]
    with pytest.raises(NotImplementedError, match="mask_size must be 0 .got 16."):
        CocoSceneGraphDataset("nowhere", inst, stuff, mask_size=16)


def test_more_objects_than_the_graph_takes_are_refused_at_construction(tmp_path):
    from canonicalsg2im_amd.sg2im.data.coco import CocoSceneGraphDataset
    images = [{"id": 7, "file_name": "7.png", "width": 100, "height": 100}]
    row = {"image_id": 7, "category_id": 1, "bbox": [0.0, 0.0, 50.0, 50.0], "segmentation": []}
    paths = []
    for name, cats, count in (("instances", [{"id": 1, "name": "person"}], 255), ("stuff", [{"id": 92, "name": "banner"}], 1)):
        paths.append(str(tmp_path / (name + ".json")))
        with open(paths[-1], "w") as f:
            json.dump({"images": images, "categories": cats,
                       "annotations": [dict(row, id=k, category_id=cats[0]["id"]) for k in range(count)]}, f)
    with pytest.raises(ValueError, match="image 7 keeps 256 objects; the canonical graph takes at most 255 per picture"):
        CocoSceneGraphDataset("nowhere", paths[0], paths[1], max_objects=1000)
    assert CocoSceneGraphDataset("nowhere", paths[0], paths[1], max_objects=255).image_ids == []
    assert len(CocoSceneGraphDataset("nowhere", paths[0], paths[1], max_objects=1000, min_object_size=0.3)) == 0


def test_the_command_line_names_the_dataset_and_the_val_list(tmp_path):
    from canonicalsg2im_amd.scripts.train import build_parser, folder_dataset
    from canonicalsg2im_amd.sg2im.data import FOLDER_DATASETS
    from canonicalsg2im_amd.sg2im.data.coco import CocoSceneGraphDataset
    from canonicalsg2im_amd.sg2im.data.packed_coco import PackedCocoSceneGraphDataset
    assert FOLDER_DATASETS["coco"] == ("coco", "build_coco_pairs_dataset")
    assert FOLDER_DATASETS["packed_coco"] == ("packed_coco", "build_coco_dataset")
    root = str(tmp_path / "root")
    parse = lambda *extra: build_parser().parse_args(["--dataroot", root, "--image_size", "64,64"] + list(extra))
    assert parse().dataset == "coco" and folder_dataset(parse(), "train") is None              # no folder: synthetic, as before
    image_dir, _ = pc.write_folder(root)
    pc.write_folder(root, split="val")
    ds = folder_dataset(parse(), "train")
    assert type(ds) is CocoSceneGraphDataset and ds.image_dir == image_dir and ds.image_ids == [13, 14, 15]     # 3 .. 8 objects
    assert ds.include_relationships and not ds.use_converse and ds.vocab == pc.vocab()
    ds = folder_dataset(parse("--min_objects", "1", "--max_objects", "5", "--use_converse", "1", "--include_relationships", "0"),
                        "train")
    assert ds.image_ids == [11, 12, 13, 14] and ds.use_converse and not ds.include_relationships
    packed = folder_dataset(parse("--dataset", "packed_coco", "--min_objects", "1"), "train")
    assert type(packed) is PackedCocoSceneGraphDataset and packed.image_ids == [11, 12, 13, 14, 15]
    ids = str(tmp_path / "val_ids.json")
    with open(ids, "w") as f:
        json.dump([15, 12, 99], f)
    assert folder_dataset(parse("--min_objects", "1"), "val").image_ids == [11, 12, 13, 14, 15]
    assert folder_dataset(parse("--min_objects", "1", "--coco_val_ids", ids), "val").image_ids == [12, 15]
    assert folder_dataset(parse("--min_objects", "1", "--coco_val_ids", ids), "train").image_ids == [11, 12, 13, 14, 15]
    with open(ids, "w") as f:
        json.dump({"ids": [12]}, f)
    with pytest.raises(ValueError, match="a JSON list of image ids is expected"):
        folder_dataset(parse("--coco_val_ids", ids), "val")
    with pytest.raises(NotImplementedError, match="mask_size must be 0 .got 16."):
        folder_dataset(parse("--mask_size", "16"), "train")
    assert os.path.isdir(image_dir)


def test_annotations_are_the_reference_boxes_bit_for_bit(tmp_path):
    """x / WW, y / HH, w / WW, h / HH in double, rounded once to fp32 (coco.py:319-322), over the decoded size."""
    from canonicalsg2im_amd.sg2im.data.coco import CocoSceneGraphDataset
    root = str(tmp_path)
    image_dir, _ = pc.write_folder(root)
    ann = os.path.join(root, "MSCoco", "annotations")
    ds = CocoSceneGraphDataset(image_dir, os.path.join(ann, "instances_train2017.json"), os.path.join(ann, "stuff_train2017.json"),
                               min_objects=1)
    _, _, g = pc.case_arrays(0, 0)
    sizes = pc.golden()[1]["sizes"]
    for b in range(5):
        n = int(g["n"][b])
        objs, boxes = ds.annotations(b, int(sizes[b, 1]), int(sizes[b, 0]))
        assert np.array_equal(objs, g["objs"][b, :n]) and boxes.dtype == np.float32
        assert np.array_equal(boxes.view(np.uint32), g["boxes"][b, :n].view(np.uint32))
