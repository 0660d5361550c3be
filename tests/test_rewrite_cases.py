"""The restatements of graph rewriting and layout consistency (tests/rewrite_cases.py) against fixed vectors, against the
golden scenes (tests/golden/clevr_syn.npz: `one_sided` is an exact equivalence under the datasets' pair rule, whose
restatement tests/test_agreement_cases.py holds to the reference's verdicts) and against hand-made layouts; the coverage of
the case tables the device is held to (tests/test_gpu_rewrite.py); and what the Python layer refuses on the host.  CPU only;
every comparison is exact."""
import math

import numpy as np
import pytest
import torch

import agreement_cases as ac
import rewrite_cases as rc
from conftest import load_golden


@pytest.fixture(scope="module")
def scenes():
    """[(rows (n,3) of the minimal graph's location rows, boxes (O,4), centers (O,2))] of the golden batches, and the table"""
    meta, z = load_golden("clevr_syn")
    table = meta["pred_name_to_idx"]
    out = []
    for run in meta["runs"]:
        if run.get("getitem"):
            continue
        pre = "%s_lt0_" % run["key"]
        triplets, ttype = z[pre + "triplets"].numpy().astype(np.int64), z[pre + "triplet_type"].numpy().astype(np.int64)
        boxes, centers = z[pre + "boxes"].numpy(), z[pre + "centers"].numpy()
        rows, counts = rc.restate_select(triplets, ttype, table, boxes.shape[1])
        assert (counts > 0).all()
        out.extend((rows[b, :counts[b]], boxes[b], centers[b]) for b in range(len(counts)))
    assert len(out) >= 10 and sum(len(s[0]) for s in out) > 500
    return out, table


def _rewrite_one(rows, image_id, table, mode, share, direction="random", seed=0):
    return rc.restate_rewrite(rows[None], [len(rows)], [image_id], table, mode, share, direction, seed)[0]


def test_hash_equals_its_fixed_vectors():
    assert rc.step_py(0, 0) == 0xe220a8397b1dcdaf                # splitmix64's first output from state 0, as published
    for seed, image, a, b, slot, h, g in rc.HASH_VECTORS:
        assert rc.hash_py(seed, image, a, b, slot) == h and rc.step_py(h, 1) == g
        got = rc.hash_np(seed, np.int64(image), np.int64(a), np.int64(b), np.int64(slot))
        assert got.dtype == np.uint64 and int(got) == h and int(rc.step_np(got, np.uint64(1))) == g
    many = rc.hash_np(3, np.arange(4, dtype=np.int64)[:, None], np.arange(5, dtype=np.int64)[None], np.int64(2), np.int64(4))
    assert many.shape == (4, 5) and all(int(many[i, j]) == rc.hash_py(3, i, j, 2, 4) for i in range(4) for j in range(5))
    assert [rc.threshold(s) for s in (0.0, 0.5, 1.0, 2.0 ** -33, 2.0 ** -34)] == [0, 1 << 31, 1 << 32, 1, 0]


@pytest.mark.parametrize("direction", ["forward", "backward", "random"])
@pytest.mark.parametrize("share", [0.0, 0.5, 1.0])
def test_one_sided_is_an_exact_equivalence_on_the_golden_scenes(scenes, share, direction):
    samples, table = scenes
    pid = [table[n] for n in rc.SLOTS]
    forward = {pid[k] for k in rc.FORWARD_SLOTS}
    changed = total = 0
    for image_id, (rows, boxes, centers) in enumerate(samples):
        got = _rewrite_one(rows, image_id, table, "one_sided", share, direction, seed=11)
        assert got.shape == rows.shape
        assert np.array_equal(rc.mirror_closure(got, table), rc.mirror_closure(rows, table))
        tested, agrees, _, _ = ac.restate(boxes[None], centers[None], got[None], np.zeros((1, len(got)), np.int64), table)
        assert tested.all() and agrees.all()                    # the ground truth obeys every rewritten row: no exceptions
        if share == 0.0:
            assert np.array_equal(got, rows)
        if share == 1.0 and direction != "random":
            assert (np.isin(got[:, 1], list(forward)) == (direction == "forward")).all()
        if share == 1.0:                                        # both mirrored rows of a pair land on the same form
            assert len(np.unique(got, axis=0)) * 2 == len(rc.mirror_closure(got, table))
        changed += int((got != rows).any(1).sum())
        total += len(rows)
    if share == 0.5:                                            # about half of the rows are selected, half of those change
        assert 0.15 * total < changed < 0.35 * total
    if share == 1.0:
        assert 0.4 * total < changed < 0.6 * total


def test_noise_changes_the_share_it_says(scenes):
    samples, table = scenes
    pid = [table[n] for n in rc.SLOTS]
    changed = total = 0
    picks = np.zeros(6, np.int64)
    for image_id, (rows, _, _) in enumerate(samples):
        assert np.array_equal(_rewrite_one(rows, image_id, table, "noise", 0.0), rows)
        full = _rewrite_one(rows, image_id, table, "noise", 1.0, seed=5)
        assert np.array_equal(full[:, [0, 2]], rows[:, [0, 2]]) and (full[:, 1] != rows[:, 1]).all()
        assert np.isin(full[:, 1], pid).all()
        picks += np.bincount(np.searchsorted(np.sort(pid), full[:, 1]), minlength=6)
        half = _rewrite_one(rows, image_id, table, "noise", 0.5, seed=5)
        hit = half[:, 1] != rows[:, 1]
        assert np.array_equal(half[hit], full[hit])             # a row selected at 0.5 is selected at 1, with the same pick
        changed += int(hit.sum())
        total += len(rows)
    assert 0.4 * total < changed < 0.6 * total and (picks > 0.1 * total).all()


@pytest.mark.parametrize("mode,direction", [("one_sided", "random"), ("one_sided", "backward"), ("noise", "random")])
def test_a_scene_is_rewritten_alike_in_any_batch_and_row_order(scenes, mode, direction):
    samples, table = scenes
    three = samples[:3]
    R = max(len(s[0]) for s in three) + 2
    batch = np.zeros((3, R, 3), np.int64)
    batch[..., 1] = table["__padding__"]
    for b, (rows, _, _) in enumerate(three):
        batch[b, :len(rows)] = rows
    counts, ids = [len(s[0]) for s in three], [40, 41, 42]
    together = rc.restate_rewrite(batch, counts, ids, table, mode, 0.5, direction, seed=9)
    assert np.array_equal(together[0, counts[0]:], batch[0, counts[0]:])       # rows past the count are copied
    for b, (rows, _, _) in enumerate(three):
        alone = _rewrite_one(rows, ids[b], table, mode, 0.5, direction, seed=9)
        assert np.array_equal(together[b, :counts[b]], alone)
        order = np.random.default_rng(b).permutation(len(rows))
        assert np.array_equal(_rewrite_one(rows[order], ids[b], table, mode, 0.5, direction, seed=9), alone[order])
    # the image id and the seed are words of the hash: over all scenes each changes some row (a small scene alone need not)
    for other in ({"image_id": 100}, {"seed": 1}):
        assert any(not np.array_equal(_rewrite_one(rows, i + other.get("image_id", 0), table, mode, 0.5, direction,
                                                   seed=9 + other.get("seed", 0)),
                                      _rewrite_one(rows, i, table, mode, 0.5, direction, seed=9))
                   for i, (rows, _, _) in enumerate(samples))


def test_select_table_covers_what_it_says():
    assert {c[0] for c in rc.SELECT_CASES} == {1, 3} and {c[1] for c in rc.SELECT_CASES} == set(rc.ROW_COUNTS)
    assert len(rc.REWRITES) == 12
    negative = in_image = transitive = padding = 0
    for case in rc.SELECT_CASES:
        triplets, ttype, ids, table, O = rc.make_select_case(case)
        rows, counts = rc.restate_select(triplets, ttype, table, O)
        B, n, _ = case
        assert counts[0] == n and rows.shape == triplets.shape and ids.shape == (B,)
        for b in range(B):
            c = counts[b] if counts[b] >= 0 else -1 - counts[b]
            assert c == (n + b if n else 0)
            assert (rows[b, c:] == [0, table["__padding__"], 0]).all()
            assert np.isin(rows[b, :c, 1], [table[x] for x in rc.SLOTS]).all()
        negative += int((counts < 0).sum())
        location = np.isin(triplets[..., 1], [table[x] for x in rc.SLOTS])
        in_image += int((triplets[..., 1] == table["__in_image__"]).sum())
        transitive += int((location & (ttype != 0)).sum())
        padding += int((triplets[..., 1] == table["__padding__"]).sum())
    assert negative == 6 and in_image > 50 and transitive > 50 and padding > 50


def test_consistency_restatement_on_hand_made_layouts():
    a = np.asarray([[[0.125, 0.125, 0.75, 0.75], [0.25, 0.25, 0.25, 0.25], [0.5, 0.0, 0.25, 0.25], [0.0, 0.0, 0.5, 0.5]]], np.float32)
    counted = np.asarray([[1, 1, 1, 0]], np.uint8)
    iou, shift, per_f, per_i, tf, ti = rc.restate_consistency(a, a, counted, np.zeros(4), np.zeros(20, np.int64))
    assert iou.tolist() == [[1.0, 1.0, 1.0, 0.0]] and shift.tolist() == [[0.0] * 4] and per_f.tolist() == [[3.0, 3.0, 0.0, 3.0]]
    assert per_i[0, 19] == 6 == per_i[0, 18] and (per_i[0, 0:18:3] == per_i[0, 2:18:3]).all()
    by = dict(zip(rc.SLOTS, per_i[0, :18].reshape(6, 3)[:, 0].tolist()))
    assert by["__surrounding__"] == 1 and by["__inside__"] == 1               # 0 surrounds 1
    assert by["__left of__"] == by["__right of__"] == 2 and by["__above__"] == by["__below__"] == 2      # 2 against 0 and 1
    b = a.copy()
    b[0, 1] = (0.75, 0.25, 0.25, 0.25)                          # object 1 leaves object 0's inside, to its right
    b[0, 2, 0] = np.float32("nan")
    iou, shift, per_f, per_i, tf, ti = rc.restate_consistency(a, b, counted, tf, ti)
    assert iou[0, 0] == 1.0 and iou[0, 1] == 0.0 and shift[0, 1] == 0.5 and np.isnan(iou[0, 2]) and np.isnan(per_f[0, 0])
    assert per_i[0, 19] == 6 and per_i[0, 18] == 0                            # the NaN takes four pairs, the move the other two
    after = dict(zip(rc.SLOTS, per_i[0, :18].reshape(6, 3).tolist()))
    assert after["__surrounding__"] == [1, 0, 0] and after["__left of__"] == [2, 1, 0] and after["__right of__"] == [2, 1, 0]
    assert ti[19] == 12 and ti[18] == 6 and np.isnan(tf[0]) and tf[3] == 6.0


def test_consistency_table_covers_what_it_says():
    assert {c[0] for c in rc.CONSISTENCY_CASES} == {1, 3} and {c[1] for c in rc.CONSISTENCY_CASES} == {1, 2, 31, 64, 65, 255}
    nan = outside = empty = rounded = 0
    for case in rc.CONSISTENCY_CASES:
        a, b, counted = rc.make_consistency_case(case)
        assert a.dtype == b.dtype == np.float32 and counted.dtype == np.uint8 and a.shape == (case[0], case[1], 4)
        iou, shift, per_f, per_i, tf, ti = rc.restate_consistency(a, b, counted, np.zeros(4), np.zeros(20, np.int64))
        n = counted.sum(1).astype(np.int64)
        assert (per_i[:, 19] == n * (n - 1)).all() and (per_i[:, 18] <= per_i[:, 19]).all() and (per_f[:, 3] == n).all()
        assert (per_i[:, 2:18:3] <= np.minimum(per_i[:, 0:18:3], per_i[:, 1:18:3])).all()
        if case[2] == "identical":
            area = (rc._clamp_box(a)[..., 2] * rc._clamp_box(a)[..., 3]) > 0
            assert (iou[area & (counted == 1)] == 1.0).all() and (per_i[:, 18] == per_i[:, 19]).all()
            assert (per_i[:, 0:18:3] == per_i[:, 2:18:3]).all() and (per_i[:, 1:18:3] == per_i[:, 2:18:3]).all()
        nan += int(np.isnan(b).any())
        outside += int(((b < 0) | (b > 1)).any())
        empty += int((n == 0).any())
        for s in range(case[0]):                                # a sum that rounds: another association gives other bits
            terms = shift[s][counted[s] == 1].astype(np.float64)
            if not np.isnan(per_f[s, 2]):
                backwards = 0.0
                for t in terms[::-1]:
                    backwards += t
                rounded += int(backwards != per_f[s, 2] or math.fsum(terms) != per_f[s, 2])
    assert nan >= 4 and outside >= 16 and empty == 12 and rounded >= 4, (nan, outside, empty, rounded)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import ops
    return ops


def test_the_python_layer_refuses_by_the_arguments_name(ops):
    """Every refusal below is raised on the host, before a device pointer is asked for: the tensors are CPU tensors."""
    vocab = ac.vocab_of(ac.PACKED)
    rows, counts, ids = torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    good = dict(rows=rows, counts=counts, image_ids=ids, vocab=vocab, mode="noise", share=0.5)
    for change, what in (({"share": 1.5}, "share must be a number in \\[0, 1\\]"), ({"share": -0.1}, "share must be"),
                         ({"share": float("nan")}, "share must be"), ({"share": "1"}, "share must be"),
                         ({"mode": "shuffle"}, "mode must be one of"), ({"direction": "sideways"}, "direction must be one of"),
                         ({"seed": -1}, "seed must be"), ({"seed": 1 << 64}, "seed must be"), ({"seed": 0.5}, "seed must be"),
                         ({"image_ids": ids.to(torch.int32)}, "image_ids must be a \\(B,\\) = \\(2,\\) int64"),
                         ({"image_ids": torch.zeros(3, dtype=torch.int64)}, "image_ids must be"),
                         ({"image_ids": [0, 1]}, "image_ids must be"), ({"counts": torch.zeros(3, dtype=torch.int64)}, "counts must be"),
                         ({"rows": rows.to(torch.int32)}, "rows must be"), ({"rows": rows[..., :2]}, "rows must be"),
                         ({"vocab": ac.vocab_of({"__padding__": 0, "__in_image__": 1, "__above__": 2})},
                          "vocab lacks __below__, __left of__")):
        with pytest.raises(RuntimeError, match=what):
            ops.rewrite_rows(**dict(good, **change))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rewrite_rows(**good)
    trip, ttype = torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64)
    for args, what in (((trip.to(torch.int32), ttype, vocab), "triplets must be"), ((trip, ttype[:, :4], vocab), "triplet_type must be"),
                       ((trip, ttype, ac.vocab_of({"__padding__": 0})), "vocab lacks"), ((trip, ttype, vocab), "no CPU path")):
        with pytest.raises(RuntimeError, match=what):
            ops.select_location_rows(*args)
    with pytest.raises(RuntimeError, match="num_objs must be"):
        ops.select_location_rows(trip, ttype, vocab, num_objs=0)
    boxes, counted = torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.uint8)
    tf, ti = torch.zeros(4, dtype=torch.float64), torch.zeros(20, dtype=torch.int64)
    for args, what in (((boxes, boxes[:, :2], counted, tf, ti), "boxes_a and boxes_b must both be"),
                       ((boxes, boxes, counted.to(torch.int64), tf, ti), "counted must be"),
                       ((boxes, boxes, counted, tf.float(), ti), "totals_f must be"), ((boxes, boxes, counted, tf, ti[:19]), "totals_i must be"),
                       ((torch.zeros(1, 257, 4), torch.zeros(1, 257, 4), torch.zeros(1, 257, dtype=torch.uint8), tf, ti), "at most 256"),
                       ((boxes, boxes, counted, tf, ti), "no CPU path")):
        with pytest.raises(RuntimeError, match=what):
            ops.layout_consistency(*args)


def test_the_run_refuses_what_it_cannot_do(ops):
    from canonicalsg2im_amd.scripts import sample
    from canonicalsg2im_amd.sg2im.data.base_dataset import canonical_triplets
    from canonicalsg2im_amd.split import Rewrite, robustness_report
    for kw, what in (({"mode": "both"}, "mode must be"), ({"mode": "noise", "share": 2}, "share must be"),
                     ({"mode": "noise", "direction": "up"}, "direction must be"), ({"mode": "noise", "seed": 1 << 32}, "seed must be")):
        with pytest.raises(ValueError, match="rewrite: " + what):
            Rewrite(**kw).check()
    assert Rewrite("one_sided").check() == Rewrite("one_sided", 1.0, "random", 0)
    with pytest.raises(SystemExit, match="--rewrite noise goes with --dataset packed_clevr_syn alone"):
        sample.parse_args(["--dataset", "packed_clevr", "--rewrite", "noise"])
    with pytest.raises(SystemExit, match="--rewrite_share"):
        sample.parse_args(["--dataset", "packed_clevr_syn", "--rewrite", "noise", "--rewrite_share", "1.5"])
    with pytest.raises(ValueError, match="robustness_report: metrics and rows of generate_split\\(rewrite"):
        robustness_report({"avg_iou": 1.0}, [])
    vocab = dict(ac.vocab_of(ac.PACKED), attributes={"shape": {"__image__": 0}}, object_name_to_idx={"__image__": 0})
    with pytest.raises(ValueError, match="triplet_counts goes with boxes=None"):
        canonical_triplets(torch.zeros(1, 2, dtype=torch.int64), None, None, [2], vocab, triplets=torch.zeros(1, 1, 3, dtype=torch.int64),
                           triplet_counts=[1])


def test_robustness_report_adds_up_from_the_rows():
    from canonicalsg2im_amd.split import LOCATION_RELATIONS, robustness_report

    def pairs(n, both):
        out = {name: {"in_a": n, "in_b": n, "in_both": both} for name in LOCATION_RELATIONS}
        out.update(same_pairs=both, pairs=n)
        return out

    def row(i, n, iou, riou, cons, both):
        return {"image_id": i, "objects": ["x"] * n, "iou": [iou] * n, "rewritten": {
            "boxes_pred": [[0, 0, 1, 1]] * n, "iou": [riou] * n, "consistency_iou": [cons] * n, "shift": [0.25] * n,
            "pair_relations": pairs(n * (n - 1), both), "relation_agreement": {"agreeing": [both, 0, 0, 0], "tested": [n, 0, 0, 0]}}}

    rows = [row(0, 2, 0.5, 0.25, 1.0, 2), row(1, 2, 1.0, 0.75, 0.5, 1), row(2, 3, 0.25, 0.25, 0.75, 3)]
    summary = {"avg_iou": 0.4, "total_iou_05": 0.1, "total_iou_03": 0.2, "num_boxes": 7.0,
               "consistency": {"avg_iou": 0.75, "share_above_05": 0.7, "avg_shift": 0.25},
               "pair_relations": pairs(10, 6), "relation_agreement": {"agreeing": 6, "tested": 7}}
    metrics = {"avg_iou": 0.5, "total_iou_05": 0.3, "total_iou_03": 0.6, "num_boxes": 7.0, "rewritten": summary}
    doc = robustness_report(metrics, rows, rewrite={"mode": "noise", "share": 0.5, "direction": "random", "seed": 3}, checkpoint="c.pt")
    assert set(doc) == {"rewrite", "checkpoint", "images", "clean", "rewritten", "consistency", "pair_relations", "relation_agreement",
                        "by_num_objects"}
    assert doc["rewrite"]["mode"] == "noise" and doc["images"] == 3 and doc["clean"]["avg_iou"] == 0.5
    assert doc["rewritten"] == {k: summary[k] for k in ("avg_iou", "total_iou_05", "total_iou_03", "num_boxes")}
    by = doc["by_num_objects"]
    assert sorted(by) == ["2", "3"] and by["2"]["images"] == 2 and by["2"]["clean"]["avg_iou"] == 0.75
    assert by["2"]["rewritten"] == {"num_boxes": 4, "avg_iou": 0.5, "total_iou_05": 0.5, "total_iou_03": 0.5}
    assert by["2"]["consistency"] == {"avg_iou": 0.75, "share_above_05": 0.5, "avg_shift": 0.25}
    assert by["2"]["pair_relations"]["__inside__"] == {"in_a": 4, "in_b": 4, "in_both": 3, "kept": 0.75}
    assert by["2"]["pair_relations"]["same_pairs"] == 3 and by["2"]["pair_relations"]["same_share"] == 0.75
    assert by["3"]["relation_agreement"]["by_type"]["original"] == {"agreeing": 3, "tested": 3, "rate": 1.0}
    assert sum(v["pair_relations"]["pairs"] for v in by.values()) == 10
