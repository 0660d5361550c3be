"""The unpacked CLEVR dataset on the CPU: the bit-row restatement of its graph against the reference's recorded output
(tests/clevr_graph_cases.py, tests/golden/clevr_unpacked.npz), the case table, the vocabulary, the registry entry and the
folder dataset's host half.  Integers throughout: equality, no tolerance."""
import os

import numpy as np
import pytest

import clevr_graph_cases as gc


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clevru"))
    return root, gc.write_folder(root)


def _args(root, *more):
    from canonicalsg2im_amd.scripts.train import build_parser
    return build_parser().parse_args(["--dataset", "clevr", "--dataroot", root, "--image_size", "64,64"] + list(more))


def _bits(rows, n):
    M = [0] * n
    for s, _, o in rows:
        M[s] |= 1 << o
    return M


def test_the_golden_is_small_and_has_every_case():
    meta, g = gc.golden()
    assert meta["cases"] == list(gc.NAMES) and meta["mixed"] == list(gc.MIXED) and len(gc.NAMES) == 12
    for keep in (0, 1):
        for name in gc.NAMES + ("mixed",):
            assert "%s_k%d_triplets" % (name, keep) in g and "%s_k%d" % (name, keep) in meta["counts"]
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "clevr_unpacked.npz")) < 100 * 1024


def test_the_cases_are_the_cases_they_are_meant_to_be():
    meta, _ = gc.golden()
    counts = meta["counts"]
    right = gc.PREDS["right"]
    rows = {name: gc.rows_of(name) for name in gc.NAMES}
    per = lambda name, p: [r for r in rows[name].tolist() if r[1] == p]
    assert len(rows["one"]) == 0 and counts["one_k0"] == [1]                              # the dummy alone
    assert sorted(rows["two"][:, 1].tolist()) == [1, 2, 3, 4] and counts["two_k0"] == [6]  # one row each: as listed
    assert all(len(per("three_order", p)) == 3 for p in (1, 2, 3, 4)) and counts["three_order_k0"] == [4 * 2 + 3]
    assert len(rows["ten_orders"]) == 4 * 45 and counts["ten_orders_k0"] == [4 * 9 + 10] and counts["ten_orders_k1"] == [190]
    chains = gc.graph(rows["ten_orders"], 10, 0)[:36, [0, 2]].reshape(4, 18)
    assert len({tuple(c.tolist()) for c in chains}) == 4                                  # four different orders
    assert per("dup2", right) == [[1, right, 0]] * 2 and counts["dup2_k0"] == [2 + 3]     # duplicates kept
    assert per("dup3", right) == [[1, right, 0], [1, right, 0], [2, right, 0]] and counts["dup3_k0"] == [2 + 3]   # merged
    listed = per("listed_order", right)
    assert listed == [[2, right, 0], [0, right, 1]] and listed != sorted(listed)          # as listed is not row-major
    for name, p in (("cycle_chain", right), ("self_relation", right)):
        C = gc.closure_bits(per(name, p), gc.SCENES[name][0])
        assert len(per(name, p)) >= 3 and any(c >> i & 1 for i, c in enumerate(C)), name  # a set diagonal in the closure
    M = _bits(per("cycle_chain", right), 5)
    assert M[0] >> 1 & 1 and M[1] >> 0 & 1                                                # the 2-cycle
    assert any(s == o for s, _, o in per("self_relation", right))
    dag = per("open_dag", right)
    assert sorted((s, o) for s, _, o in dag) == [(0, 1), (0, 2), (1, 2), (2, 3)]          # a->b, b->c, a->c, c->d
    assert gc.closure_bits(dag, 4) != _bits(dag, 4) and counts["open_dag_k0"] == [3 + 4] and counts["open_dag_k1"] == [4 + 4]
    first = list(dict.fromkeys(rows["key_order"][:, 1].tolist()))
    assert first == [4, 3, 1, 2] and first != sorted(first)                               # not ascending predicate id
    assert gc.SCENES["n63"][0] == 63 and len(rows["n63"]) == 4 * 1953 and rows["n63"][:, [0, 2]].max() == 62
    assert counts["n63_k0"] == [4 * 62 + 63] and counts["n63_k1"] == [4 * 1953 + 63]
    assert [gc.SCENES[nm][0] for nm in gc.MIXED] == [1, 3, 10, 63]


@pytest.mark.parametrize("keep", [0, 1], ids=["keep0", "keep1"])
@pytest.mark.parametrize("name", gc.NAMES)
def test_restatement_equals_the_reference(name, keep):
    meta, g = gc.golden()
    n = gc.SCENES[name][0]
    got = gc.graph(gc.rows_of(name), n, keep)
    want = g["%s_k%d_triplets" % (name, keep)].astype(np.int64)
    assert want.shape[0] == 1 and [len(got)] == meta["counts"]["%s_k%d" % (name, keep)]
    assert np.array_equal(got, want[0])


@pytest.mark.parametrize("keep", [0, 1], ids=["keep0", "keep1"])
def test_restated_mixed_batch_equals_the_reference_collate(keep):
    meta, g = gc.golden()
    rows, n_objs = gc.padded_rows(gc.MIXED)
    trip, counts = gc.batch(rows, n_objs, keep)
    assert counts.tolist() == meta["counts"]["mixed_k%d" % keep] and n_objs.tolist() == [2, 4, 11, 64]
    assert np.array_equal(trip, g["mixed_k%d_triplets" % keep].astype(np.int64))
    assert (trip[0, 1:] == [0, gc.PREDS["__padding__"], 0]).all()
    boxes, objs = g["mixed_boxes"], g["mixed_objs"]
    assert boxes.shape == (4, 64, 4) and objs.shape == (4, 64, 4) and boxes.dtype == np.float32
    for b, n in enumerate(n_objs - 1):
        assert boxes[b, n].tolist() == [0, 0, 1, 1] and (boxes[b, n + 1:] == -1).all()     # clevr_dialog.py:178, :444
        assert (objs[b, n:] == 0).all() and (objs[b, :n] > 0).all()


def test_vocabulary_equals_the_recorded_one(folder):
    from canonicalsg2im_amd.sg2im.data import build_folder_dataset
    v = build_folder_dataset(_args(folder[0]), "train").vocab
    want = gc.golden()[0]["vocab"]
    assert v["pred_name_to_idx"] == want["pred_name_to_idx"] == gc.PREDS
    assert v["pred_idx_to_name"] == want["pred_idx_to_name"] and isinstance(v["pred_idx_to_name"], list)
    assert v["attributes"] == want["attributes"] and list(v["attributes"]) == list(want["attributes"])
    assert v["object_name_to_idx"] == want["object_name_to_idx"] and list(v["object_name_to_idx"]) == list(want["object_name_to_idx"])
    assert v["use_object_embedding"] is False and v["reverse_attributes"]["color"][8] == "yellow"
    assert v["object_idx_to_name"][0] == "__image__"


def test_command_line_builds_the_dataset(folder, tmp_path):
    from canonicalsg2im_amd.sg2im.data import FOLDER_DATASETS, build_folder_dataset, looked_for
    from canonicalsg2im_amd.sg2im.data.clevr import CLEVRDialogDataset, ClevrDialogBatchBuilder
    from canonicalsg2im_amd.sg2im.data.packed_clevr import PackedClevrDataset
    root, base = folder
    assert FOLDER_DATASETS["clevr"] == ("clevr", "build_clevr_dialog_dataset")
    ds = build_folder_dataset(_args(root), "train")
    assert isinstance(ds, CLEVRDialogDataset) and isinstance(ds, PackedClevrDataset)
    assert ds.builder_class is ClevrDialogBatchBuilder and len(ds) == 4 and ds.image_ids == [10, 12, 13, 21]
    assert ds.image_dir == os.path.join(base, "images") and ds.image_size == (64, 64) and ds.use_transitivity == 0
    with ds.open(1) as im:
        assert im.size == (53, 37) and im.mode == "RGB"
    for i, name in enumerate(gc.MIXED):
        objs, geom, rot, rows = ds.annotations(i)
        assert rows.dtype == np.int64 and np.array_equal(rows, gc.rows_of(name)) and objs.shape == (gc.SCENES[name][0], 4)
    assert build_folder_dataset(_args(root), "val") is None                              # no val pictures
    nowhere = str(tmp_path / "nowhere")
    assert build_folder_dataset(_args(nowhere), "train") is None                         # the trainer keeps its synthetic batches
    assert looked_for(_args(nowhere), "train") == os.path.join(nowhere, "CLEVR", "CLEVR_Dialog", "images", "train")
    # the reference's dense filter keeps the scenes of MORE than max_objects objects (clevr_dialog.py:192-199)
    ds = build_folder_dataset(_args(root, "--dense_scenes", "1", "--max_objects", "3", "--use_transitivity", "1"), "train")
    assert ds.image_ids == [13, 21] and ds.use_transitivity == 1 and [os.path.basename(p) for p in ds.image_paths] == [
        "CLEVR_train_000013.png", "CLEVR_train_000021.png"]
    ds = build_folder_dataset(_args(nowhere, "--clevr_train_image_dir", os.path.join(base, "images", "train"),
                                    "--clevr_train_scenes_json", os.path.join(base, "scenes", "CLEVR_train_scenes.json"),
                                    "--num_train_samples", "3"), "train")
    assert len(ds) == 3 and ds.image_dir == os.path.join(base, "images", "train")


def test_refusals(folder, tmp_path):
    import json
    from canonicalsg2im_amd.sg2im.data import build_folder_dataset
    from canonicalsg2im_amd.sg2im.data.clevr import CLEVRDialogDataset
    root, base = folder
    for flag in ("--learned_transitivity", "--learned_converse", "--use_converse"):
        with pytest.raises(ValueError, match="%s is not part of.*packed_clevr" % flag[2:]):
            build_folder_dataset(_args(root, flag, "1"), "train")
    with pytest.raises(NotImplementedError, match="mask_size must be 0.*packed_clevr"):
        build_folder_dataset(_args(root, "--mask_size", "16"), "train")
    with pytest.raises(ValueError, match="use_transitivity must be 0 or 1"):
        build_folder_dataset(_args(root, "--use_transitivity", "2"), "train")
    scenes = os.path.join(base, "scenes", "CLEVR_train_scenes.json")
    with pytest.raises(ValueError, match="use_transitivity must be 0 or 1"):
        CLEVRDialogDataset(scenes, os.path.join(base, "images"), use_transitivity=0.5)
    with open(scenes) as f:
        doc = json.load(f)
    bad = str(tmp_path / "bad.json")
    for what, edit, msg in (("index", lambda s: s["relationships"]["right"][0].append(3), "names object 3 outside"),
                            ("negative", lambda s: s["relationships"]["left"][2].append(-1), "names object -1 outside"),
                            ("key", lambda s: s["relationships"].update(above=[[], [], []]), "'above' is no predicate"),
                            ("short", lambda s: s["relationships"]["front"].pop(), "has 2 lists for 3 objects")):
        changed = json.loads(json.dumps(doc))
        edit(changed["scenes"][1])                                                       # three_order: 3 objects
        with open(bad, "w") as f:
            json.dump(changed, f)
        ds = CLEVRDialogDataset(bad, os.path.join(base, "images"))
        assert len(ds.annotations(0)[3]) == 0
        with pytest.raises(ValueError, match=msg):
            ds.annotations(1)
    many = json.loads(json.dumps(doc))
    many["scenes"][3]["objects"].append(dict(many["scenes"][3]["objects"][0]))             # 64 objects
    with open(bad, "w") as f:
        json.dump(many, f)
    with pytest.raises(ValueError, match="a scene has 64 objects, at most 63"):
        CLEVRDialogDataset(bad, os.path.join(base, "images"))
